"""CPU-side checks of the bounded TV-LQR beyond the LDS horizon (csrc/boxqp.hip with its factor records in a
workspace in HBM): the size queries and the argument checks of the workspace entries.  No GPU is touched."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 160 * 1024 - 512
QUAD, BICYCLE, HAND, BOX_PIVOT = 1, 2, 4, 5


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from irs_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.load()


def test_workspace_bytes_quadrotor(lib):
    assert lib.irs_tvlqr_box_workspace_bytes(QUAD, 50, 0) == 0                # T = 50 still fits on chip
    assert lib.irs_tvlqr_box_lds_bytes(QUAD, 50) <= LDS_LIMIT
    assert lib.irs_tvlqr_box_workspace_bytes(QUAD, 51, 0) > 0
    assert lib.irs_tvlqr_box_workspace_bytes(QUAD, 200, 0) >= 200 * 340 * 8    # one 340-double record per step
    assert lib.irs_tvlqr_box_workspace_bytes(QUAD, 200, 0) % 256 == 0
    assert 0 < lib.irs_tvlqr_box_hbm_lds_bytes(QUAD, 200, 0) <= LDS_LIMIT
    assert lib.irs_tvlqr_box_workspace_bytes(QUAD, 200, 1) == 0               # the quadrotor has no du form
    assert lib.irs_tvlqr_box_hbm_lds_bytes(QUAD, 200, 1) == 0


def test_workspace_bytes_position_controlled(lib):
    assert lib.irs_tvlqr_box_workspace_bytes(HAND, 80, 1) > 0                 # planar hand, du form: beyond T = 56
    assert 0 < lib.irs_tvlqr_box_hbm_lds_bytes(HAND, 80, 1) <= LDS_LIMIT
    assert lib.irs_tvlqr_box_workspace_bytes(BOX_PIVOT, 120, 1) == 0          # box pivoting, du form: on chip
    # solver 1 of the quasistatic descent: the records beyond LDS (0 wherever they fit, as before)
    assert lib.irs_quasistatic_descent_workspace_bytes(HAND, 50, 1) == 0
    assert lib.irs_quasistatic_descent_workspace_bytes(HAND, 80, 1) == lib.irs_tvlqr_box_workspace_bytes(HAND, 80, 1)
    assert lib.irs_quasistatic_descent_workspace_bytes(BOX_PIVOT, 120, 1) == 0


def test_the_new_horizon_limits(lib):
    def cap(model, du):
        T = 1
        while 0 < lib.irs_tvlqr_box_hbm_lds_bytes(model, T + 1, du) <= LDS_LIMIT:
            T += 1
        return T
    # the reference's scripts: quadrotor T = 200, bicycle 100, planar hand / box pivoting well below these
    assert cap(QUAD, 0) == 357 and cap(BICYCLE, 0) == 867
    assert cap(HAND, 1) == 383 and cap(BOX_PIVOT, 1) == 679
    assert lib.irs_tvlqr_box_hbm_lds_bytes(QUAD, 358, 0) > LDS_LIMIT          # past the cap: unsupported
    assert lib.irs_tvlqr_box_hbm_lds_bytes(HAND, 384, 1) > LDS_LIMIT


def test_iterate_scratch_grows_only_beyond_the_lds_horizon(lib):
    exact = 3
    small = lib.irs_iterate_scratch_bytes(QUAD, exact, 50, 0)
    big = lib.irs_iterate_scratch_bytes(QUAD, exact, 100, 0)
    assert big >= small + lib.irs_tvlqr_box_workspace_bytes(QUAD, 100, 0)
    assert lib.irs_iterate_scratch_bytes(QUAD, 0, 100, 1000) >= lib.irs_tvlqr_box_workspace_bytes(QUAD, 100, 0)


def test_device_model_support_queries(lib):
    from irs_mpc_amd import systems
    dq = systems.QuadrotorDynamics(0.05).dm()
    assert dq.box_descent_supported(50) and dq.box_descent_supported(200) and dq.box_descent_supported(357)
    assert not dq.box_descent_supported(358)
    assert dq.box_horizon_limit() == 357
    dh = systems.PlanarHandDynamics(0.1).dm()
    assert dh.quasistatic_descent_supported(80, 1) and dh.quasistatic_descent_supported(383, 1)
    assert not dh.quasistatic_descent_supported(384, 1)
    assert dh.box_horizon_limit(du=True) == 383


def test_wsx_argument_checks_without_gpu(lib):
    from irs_mpc_amd._lib import dbl_array
    bike = dbl_array([0.1])
    ph = dbl_array([0.1, 10.0, 1.0, 0.25, 0.5, 50.0, 25.0, 0.3, 0.2, 0.05, 0.1, 50.0])
    one = 8             # any non-null address: validation happens before anything is dereferenced
    ws = 256            # a 256-byte aligned one
    a = [one] * 6
    # irs_tvlqr_box_descent_wsx: null pointers, a workspace too small for the records, a misaligned one
    assert lib.irs_tvlqr_box_descent_wsx(BICYCLE, bike, 1, 30, None, *a[:5], 0.5, one, one, one, one, one, one,
                                         10.0, 1.6, 100, 1e-8, one, one, one, ws, 1 << 20, None) == -1
    assert lib.irs_tvlqr_box_descent_wsx(BICYCLE, bike, 1, 30, *a, 0.5, one, one, one, one, one, one,
                                         10.0, 1.6, 100, 1e-8, None, one, one, ws, 1 << 20, None) == -1
    assert lib.irs_tvlqr_box_descent_wsx(BICYCLE, bike, 1, 30, *a, 0.5, one, one, one, one, one, one,
                                         10.0, 1.6, 100, 1e-8, one, one, one, ws, 30 * 74 * 8 - 8, None) == -4
    assert b"workspace" in lib.irs_last_error()
    assert lib.irs_tvlqr_box_descent_wsx(BICYCLE, bike, 1, 30, *a, 0.5, one, one, one, one, one, one,
                                         10.0, 1.6, 100, 1e-8, one, one, one, ws + 8, 1 << 20, None) == -1
    # irs_tvlqr_box_solve_wsx, position-controlled planar hand
    assert lib.irs_tvlqr_box_solve_wsx(HAND, ph, 12, 10, None, *a[:5], 1.0, one, one, 1, None, None, one, one,
                                       None, None, 100.0, 1.6, 100, 1e-8, one, one, one, ws, 1 << 20, None) == -1
    assert lib.irs_tvlqr_box_solve_wsx(HAND, ph, 12, 10, *a, 1.0, one, one, 1, None, None, one, one,
                                       None, None, 100.0, 1.6, 100, 1e-8, one, one, None, ws, 1 << 20, None) == -1
    assert lib.irs_tvlqr_box_solve_wsx(HAND, ph, 12, 10, *a, 1.0, one, one, 1, None, None, one, one,
                                       None, None, 100.0, 1.6, 100, 1e-8, one, one, one, ws, 10 * 302 * 8 - 8,
                                       None) == -4
    # the bicycle has no position-controlled form
    assert lib.irs_tvlqr_box_solve_wsx(BICYCLE, bike, 1, 10, *a, 1.0, one, one, 1, None, None, one, one,
                                       None, None, 100.0, 1.6, 100, 1e-8, one, one, one, ws, 1 << 20, None) == -3
