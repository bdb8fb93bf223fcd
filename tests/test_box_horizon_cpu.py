"""CPU-side checks of the bounded TV-LQR beyond the LDS horizon (csrc/boxqp.hip with its factor records in a
workspace in HBM): the size queries, the placement table of the bounded descents and the argument checks of the
workspace entries.  No GPU is touched: every call is a size query or is rejected before any HIP call."""
import ctypes
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 160 * 1024 - 512
QUAD, BICYCLE, HAND, BOX_PIVOT = 1, 2, 4, 5
N_MODELS = 11
INT_MAX = 2 ** 31 - 1
GOLDEN = os.path.join(ROOT, "tests", "golden", "box_plan_table.json")


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
    # the legacy entries: the same checks before anything runs
    assert lib.irs_tvlqr_box_descent(BICYCLE, bike, 1, 30, None, *a[:5], 0.5, one, one, one, one, one, one,
                                     10.0, 1.6, 100, 1e-8, one, one, one, None) == -1
    assert lib.irs_tvlqr_box_descent(BICYCLE, bike, 1, 30, *a, 0.5, one, one, one, one, one, one,
                                     10.0, 2.0, 100, 1e-8, one, one, one, None) == -1        # relax < 2
    assert lib.irs_tvlqr_box_descent_if(BICYCLE, bike, 1, 30, *a, 0.5, one, one, one, one, one, one,
                                        10.0, 1.6, 100, 1e-8, one, one, None, None, None, None) == -1
    assert lib.irs_tvlqr_box_descent_if(11, bike, 1, 30, *a, 0.5, one, one, one, one, one, one,
                                        10.0, 1.6, 100, 1e-8, one, one, None, one, None, None) == -3
    assert b"unknown model" in lib.irs_last_error()
    assert lib.irs_tvlqr_box_solve(HAND, ph, 12, 10, None, *a[:5], 1.0, one, one, 1, None, None, one, one,
                                   None, None, 100.0, 1.6, 100, 1e-8, one, one, one, None) == -1
    assert lib.irs_tvlqr_box_solve(BICYCLE, bike, 1, 10, *a, 1.0, one, one, 1, None, None, one, one,
                                   None, None, 100.0, 1.6, 100, 1e-8, one, one, one, None) == -3
    # past the caps: the plain form at T = 358 on the quadrotor, with or without a workspace
    nq = lib_nparams(lib, QUAD)
    quad = dbl_array([0.1] * nq)
    assert lib.irs_tvlqr_box_descent_wsx(QUAD, quad, nq, 358, *a, 0.5, one, one, one, one, one, one,
                                         10.0, 1.6, 100, 1e-8, one, one, one, ws, 1 << 30, None) == -3
    assert lib.irs_tvlqr_box_descent(QUAD, quad, nq, 51, *a, 0.5, one, one, one, one, one, one,
                                     10.0, 1.6, 100, 1e-8, one, one, one, None) == -3
    assert b"workspace" in lib.irs_last_error()
    # irs_quasistatic_box_descent_ws / _wsx: null pointers, an unknown solver, two boxes for the active set, a
    # model that is not position controlled, horizons the chosen solver cannot take
    q = [one] * 8
    assert lib.irs_quasistatic_box_descent_ws(HAND, ph, 12, 10, None, *q[:7], None, None, None, None, None, None,
                                              0, 10.0, 1.6, 100, 1e-8, one, one, None, one, None, None) == -1
    assert lib.irs_quasistatic_box_descent_ws(HAND, ph, 12, 10, *q, None, None, None, None, None, None,
                                              4, 10.0, 1.6, 100, 1e-8, one, one, None, one, None, None) == -1
    assert lib.irs_quasistatic_box_descent_ws(HAND, ph, 12, 10, *q, None, None, one, one, one, one,
                                              3, 10.0, 1.6, 100, 1e-8, one, one, None, one, None, None) == -3
    for solver in (1, 2, 3):
        assert lib.irs_quasistatic_box_descent_wsx(BICYCLE, bike, 1, 10, *q, None, None, one, one, None, None, solver,
                                                   10.0, 1.6, 100, 1e-8, one, one, None, one, None, None, 0,
                                                   None) == -3
        assert b"position controlled" in lib.irs_last_error()
    assert lib.irs_quasistatic_box_descent_ws(HAND, ph, 12, 80, *q, None, None, one, one, None, None,
                                              2, 10.0, 1.6, 100, 1e-8, one, one, None, one, None, None) == -3
    assert lib.irs_quasistatic_box_descent_wsx(HAND, ph, 12, 120, *q, None, None, one, one, None, None, 3,
                                               10.0, 1.6, 100, 1e-8, one, one, None, one, None, ws, 256, None) == -3
    assert b"workspace" in lib.irs_last_error()
    assert lib.irs_quasistatic_box_descent_ws(HAND, ph, 12, 384, *q, None, None, one, one, one, one,
                                              1, 10.0, 1.6, 100, 1e-8, one, one, None, one, None, None) == -3


def lib_nparams(lib, model):
    n = ctypes.c_int()
    assert lib.irs_model_info(model, None, None, ctypes.byref(n)) == 0
    return n.value


def walk_horizon_limit(lib, model, kind):
    """The longest horizon the size queries let `kind` run, by walking T upwards (0: the model has no such form)."""
    if kind == 3:
        return INT_MAX if lib.irs_quasistatic_box_lds_bytes(model, 1, 3) > 0 else 0
    if kind == 2:
        def fits(T):
            return 0 < lib.irs_quasistatic_box_lds_bytes(model, T, 2) <= LDS_LIMIT
    else:
        def fits(T):
            return 0 < lib.irs_tvlqr_box_hbm_lds_bytes(model, T, kind) <= LDS_LIMIT
    T = 0
    while fits(T + 1):
        T += 1
    return T


def plan_horizons(lib, model):
    """T = 0..64, a stride to ~1100 and each cap +-1: the caps with records in HBM, and where the records leave LDS."""
    caps = [walk_horizon_limit(lib, model, k) for k in range(3)]
    for fits in (lambda T: lib.irs_tvlqr_box_lds_bytes(model, T) <= LDS_LIMIT,
                 lambda T: 0 < lib.irs_quasistatic_box_lds_bytes(model, T, 1) <= LDS_LIMIT,
                 lambda T: 0 < lib.irs_quasistatic_box_lds_bytes(model, T, 3) <= LDS_LIMIT):
        T = 0
        while T < 2000 and fits(T + 1):
            T += 1
        caps.append(T)
    Ts = set(range(65)) | set(range(80, 1101, 40)) | {c + d for c in caps if c > 0 for d in (-1, 0, 1)}
    return sorted(Ts)


def box_plan_table(lib, horizons=None):
    """Every placement answer of the bounded descents for the 11 models: the size queries of csrc/boxqp.hip, the fused
    iterate's scratch (modes 0-3, N = 1000) and DeviceModel's support answers.  horizons: {model: [T, ...]}."""
    from irs_mpc_amd.device import DeviceModel
    table = {}
    for model in range(N_MODELS):
        Ts = horizons[str(model)] if horizons else plan_horizons(lib, model)
        dm = DeviceModel(model, [0.1] * lib_nparams(lib, model))
        row = {"T": Ts,
               "tvlqr_box_lds_bytes": [lib.irs_tvlqr_box_lds_bytes(model, T) for T in Ts],
               "box_horizon_limit": [dm.box_horizon_limit(du=False), dm.box_horizon_limit(du=True)]}
        for du in (0, 1):
            row["tvlqr_box_workspace_bytes/%d" % du] = [lib.irs_tvlqr_box_workspace_bytes(model, T, du) for T in Ts]
            row["tvlqr_box_hbm_lds_bytes/%d" % du] = [lib.irs_tvlqr_box_hbm_lds_bytes(model, T, du) for T in Ts]
            row["box_descent_supported/%d" % du] = [int(dm.box_descent_supported(T, du=bool(du))) for T in Ts]
        for solver in range(4):
            row["quasistatic_box_lds_bytes/%d" % solver] = [lib.irs_quasistatic_box_lds_bytes(model, T, solver)
                                                            for T in Ts]
            row["quasistatic_descent_workspace_bytes/%d" % solver] = [
                lib.irs_quasistatic_descent_workspace_bytes(model, T, solver) for T in Ts]
            row["iterate_scratch_bytes/%d" % solver] = [lib.irs_iterate_scratch_bytes(model, solver, T, 1000)
                                                        for T in Ts]
        for solver in (1, 2, 3):
            row["quasistatic_descent_supported/%d" % solver] = [int(dm.quasistatic_descent_supported(T, solver))
                                                                for T in Ts]
        table[str(model)] = row
    return table


def test_box_plan_table_matches_the_golden(lib):
    """The planner answers every size and support question as the code before it did (tests/golden/
    box_plan_table.json was written by this module's __main__ against a library built before the planner)."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = box_plan_table(lib, {m: golden[m]["T"] for m in golden})
    assert sorted(got) == sorted(golden)
    for m in golden:
        for key in golden[m]:
            assert got[m][key] == golden[m][key], (m, key)


def test_box_horizon_limit_equals_the_walk(lib):
    from irs_mpc_amd.device import DeviceModel
    assert DeviceModel.BOX_LDS_LIMIT == LDS_LIMIT
    for model in range(N_MODELS):
        for kind in range(4):
            assert lib.irs_box_horizon_limit(model, kind) == walk_horizon_limit(lib, model, kind), (model, kind)
    assert lib.irs_box_horizon_limit(QUAD, 0) == 357 and lib.irs_box_horizon_limit(HAND, 1) == 383
    assert lib.irs_box_horizon_limit(HAND, 4) == 0 and lib.irs_box_horizon_limit(N_MODELS, 0) == 0


PENDULUM = 0
KIND_ADMM, KIND_ADMM_DU, KIND_ACTIVE_SET, KIND_TILES = 0, 1, 2, 3


def round256(v):
    return (v + 255) // 256 * 256


def test_records_bytes_is_the_planner_at_any_horizon(lib):
    """irs_box_records_bytes: what the workspace queries answer where they answer at all, and the same function of T
    below the LDS horizon, where they answer 0."""
    Ts = (1, 10, 50, 80, 200)
    for model in (HAND, BOX_PIVOT, BICYCLE, QUAD, PENDULUM):
        for kind in (KIND_ADMM, KIND_ADMM_DU, KIND_TILES):
            has_form = lib.irs_box_horizon_limit(model, kind) > 0
            got = [lib.irs_box_records_bytes(model, T, kind) for T in Ts]
            if kind == KIND_TILES:
                beyond = [lib.irs_quasistatic_descent_workspace_bytes(model, T, 3) for T in Ts]
            else:
                beyond = [lib.irs_tvlqr_box_workspace_bytes(model, T, kind) for T in Ts]
            for T, g, w in zip(Ts, got, beyond):
                assert w == 0 or g == w, (model, kind, T, g, w)
                assert (g > 0) == has_form, (model, kind, T, g)
            assert got == sorted(got), (model, kind, got)
            if kind == KIND_TILES:
                for T, g, w in zip(Ts, got, beyond):
                    for B in (1, 3):
                        batch = lib.irs_quasistatic_descent_batch_workspace_bytes(model, T, B)
                        assert batch == (B * round256(g) if w > 0 else 0), (model, T, B)
    # the forms the horizons above cover on both sides of LDS, and those that exist at all
    assert lib.irs_tvlqr_box_workspace_bytes(QUAD, 50, 0) == 0 < lib.irs_tvlqr_box_workspace_bytes(QUAD, 80, 0)
    assert lib.irs_quasistatic_descent_workspace_bytes(HAND, 50, 3) == 0
    assert lib.irs_quasistatic_descent_workspace_bytes(HAND, 80, 3) > 0
    assert lib.irs_box_records_bytes(HAND, 10, KIND_ADMM_DU) > 0 and lib.irs_box_records_bytes(HAND, 10, KIND_TILES) > 0
    assert lib.irs_box_records_bytes(BICYCLE, 10, KIND_ADMM) == round256(10 * 74 * 8)   # one 74-double record per step


def test_records_bytes_is_zero_where_nothing_is_placed(lib):
    for T in (0, -3):
        for kind in range(4):
            assert lib.irs_box_records_bytes(HAND, T, kind) == 0
    assert lib.irs_box_records_bytes(N_MODELS, 10, KIND_ADMM) == 0
    assert lib.irs_box_records_bytes(-1, 10, KIND_TILES) == 0
    assert lib.irs_box_records_bytes(HAND, 10, 4) == 0 and lib.irs_box_records_bytes(HAND, 10, -1) == 0
    for model in (QUAD, BICYCLE, PENDULUM):           # not position controlled: no du form, no tile form
        assert lib.irs_box_records_bytes(model, 10, KIND_ADMM_DU) == 0
        assert lib.irs_box_records_bytes(model, 10, KIND_TILES) == 0
    for model in (HAND, BOX_PIVOT, QUAD):             # the lanes keep everything on chip
        for T in (1, 10, 50, 80, 200):
            assert lib.irs_box_records_bytes(model, T, KIND_ACTIVE_SET) == 0


def test_fused_iterate_checks_the_admm_settings_of_its_bounded_descents(lib):
    """irs_iterate with bounds refuses ADMM settings the stand-alone bounded-descent entries refuse, with their code
    and text: qp_relax outside (0, 2) (values <= 0 mean the default, so only >= 2 can be wrong).  Exact mode: the
    call is rejected before any HIP call, so dummy addresses do."""
    from irs_mpc_amd import _lib
    one, T = 256, 8
    c = _lib.IterateCall()
    c.model, c.n_params = BICYCLE, 1
    c.params[0] = 0.1
    c.mode, c.T, c.N, c.n_descents, c.alpha_R = _lib.ITERATE_EXACT, T, 0, 1, 0.5
    for name in ("Q", "Qd", "R", "xd_trj", "xlo", "xhi", "ulo", "uhi", "x_trj0", "u_trj0", "x_hist", "u_hist",
                 "cost_hist", "info_hist", "scratch"):
        setattr(c, name, one)
    c.scratch_bytes = lib.irs_iterate_scratch_bytes(BICYCLE, _lib.ITERATE_EXACT, T, 0)
    for relax in (2.0, 2.5, float("inf")):
        c.qp_relax = relax
        assert lib.irs_iterate(ctypes.byref(c), None, None) == -1, relax
        assert lib.irs_last_error() == b"irs_tvlqr_box_descent_ifw: bad ADMM parameter"


if __name__ == "__main__":
    # writes the golden table: run from a tree whose package and library predate the planner
    sys.path.insert(0, os.getcwd())
    from irs_mpc_amd import _lib
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:
        json.dump(box_plan_table(_lib.load()), f, separators=(",", ":"))
        f.write("\n")
