"""Batched bounded TV-LQR on the device: irs_tvlqr_box_descent_batch bit for bit against B single bounded descents
(irs_tvlqr_box_descent_if with its records on chip, irs_tvlqr_box_descent_wsx with them in HBM), its run_flag, a failing
problem beside healthy ones, and IrsLqrBatch(bounded=True) against B runs of the single classes.

The cases (each converges well inside 5000 ADMM iterations with its bound active on the CPU oracle's local_descent_box,
rho 10, eps 1e-8, exact linearisation along the rollout of the initial guess):
    bicycle    h 0.1, T = 12, starts x0[1] = 0.1 b, guesses [0.1 + 0.05 b, 0]; steer within +-pi/4
    pendulum   h 0.05, T = 10, starts [0.1 b, 0], guesses 0.1 + 0.02 b; |u| <= 0.2
    quadrotor  h 0.05, T = 6, starts x0[2] = 0.05 b, guesses 2.0 + 0.1 b; thrusts in [1.0, 2.6], no attitude bound
"""
import functools

import numpy as np
import pytest
import torch

from oracle import irs_oracle as orc

pytestmark = pytest.mark.gpu

SENTINEL, INFO_SENTINEL = -777.0, -7
KEYS = ("x_new", "u_new", "cost", "info")
# tests/test_gpu_parity.py:515 -- two loops on f32 statistics: rtol on cost_lst (tests/test_irs_lqr_batch_gpu.py)
LOOP_RTOL = 1e-4
CLS_T, CLS_N, CLS_ITERS, BOUND = 10, 2500, 3, 1
QP_FAILED = "TV_LQR failed. Optimization problem is not solved."


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()     # fails loudly if the HIP library is missing
    return irs_mpc_amd


def npy(t):
    return t.detach().cpu().numpy()


def device_system(amd, name):
    return {"pendulum": amd.PendulumDynamics(0.05), "quadrotor": amd.QuadrotorDynamics(0.05),
            "bicycle": amd.BicycleDynamics(0.1)}[name]


# ---------------------------------------------------------------- the cases, host side, built once
def bike_weights():
    return np.diag([5, 5, 3, 0.1, 0.1]), np.diag([50., 50, 30, 1, 1]), np.diag([1, 0.1])


def starts(name, b):
    """(x0, u_trj_initial, xd_trj) of problem b."""
    if name == "bicycle":
        T = 12
        x0 = np.zeros(5)
        x0[1] = 0.1 * b
        return x0, np.tile(np.array([0.1 + 0.05 * b, 0.0]), (T, 1)), np.tile(np.array([3.0, 1.0, np.pi / 2, 0, 0]), (T + 1, 1))
    if name == "pendulum":
        T = CLS_T
        return np.array([0.1 * b, 0.0]), np.tile(np.array([0.1 + 0.02 * b]), (T, 1)), np.tile(np.array([np.pi, 0.0]), (T + 1, 1))
    T = 6
    x0 = np.zeros(12)
    x0[2] = 0.05 * b
    xd = np.zeros((T + 1, 12))
    for i in range(T + 1):
        xd[i, :3] = [1.5 * np.cos(0.05 * i), 1.5 * np.sin(0.05 * i), 0.02 * i]
    return x0, np.tile(np.full(4, 2.0 + 0.1 * b), (T, 1)), xd


@functools.lru_cache(maxsize=None)
def kernel_case(name):
    """Three problems of one model as the batched entry takes them: numpy blocks, the box of each problem, the shared
    weights; `bound` = (array the bound is on, component, lo, hi) for the "bound reached" check."""
    inf = np.inf
    so = {"bicycle": orc.BicycleOracle(0.1), "pendulum": orc.PendulumOracle(0.05), "quadrotor": orc.QuadrotorOracle(0.05)}[name]
    n, m = so.dim_x, so.dim_u
    blocks = {k: [] for k in ("At", "Bt", "ct", "xd", "x0")}
    for b in range(3):
        x0, u0, xd = starts(name, b)
        X = orc.rollout(so, x0, u0)
        At, Bt, ct = orc.exact_TV(so, X, u0)
        for k, v in zip(("At", "Bt", "ct", "xd", "x0"), (At, Bt, ct, xd, x0)):
            blocks[k].append(v)
    c = {k: np.stack(v) for k, v in blocks.items()}
    xlo, xhi, ulo, uhi = np.full((3, n), -inf), np.full((3, n), inf), np.full((3, m), -inf), np.full((3, m), inf)
    if name == "bicycle":
        c["Q"], c["Qd"], c["R"] = bike_weights()
        xlo[:, 4], xhi[:, 4] = -np.pi / 4, np.pi / 4
        c["bound"] = ("x_new", 4, -np.pi / 4, np.pi / 4)
    elif name == "pendulum":
        c["Q"], c["Qd"], c["R"] = np.diag([1., 1.]), np.diag([20., 20.]), np.diag([1.])
        ulo[:], uhi[:] = -0.2, 0.2
        c["bound"] = ("u_new", 0, -0.2, 0.2)
    else:
        c["Q"] = np.diag([10., 10, 10, 10, 10, 10, 0, 0, 0, 0, 0, 0])
        c["Qd"] = 10.0 * np.diag([10., 10, 10, 10, 10, 10, 1, 1, 1, 1, 1, 1])
        c["R"] = np.eye(4)
        ulo[:], uhi[:] = 1.0, 2.6
        c["bound"] = ("u_new", slice(None), 1.0, 2.6)
    c.update(xlo=xlo, xhi=xhi, ulo=ulo, uhi=uhi)
    return c


ARRAYS = ("At", "Bt", "ct", "Q", "Qd", "R", "xd", "x0", "xlo", "xhi", "ulo", "uhi")


def on_device(c, order=(0, 1, 2), **replace):
    """The blocks of problems `order` on the device (a problem may appear twice); `replace`: other arrays."""
    from irs_mpc_amd import device as dev
    d = {}
    for k in ARRAYS:
        a = replace.get(k, c[k])
        d[k] = dev.to_dev(a if k in ("Q", "Qd", "R") else a[list(order)])
    return d


def single_if(dm, d, b, **qp):
    """irs_tvlqr_box_descent_if on problem b's blocks: cost given, run_flag null, outputs prefilled."""
    from irs_mpc_amd import device as dev
    from irs_mpc_amd._lib import check
    T, device = d["At"].shape[1], d["At"].device
    o = dict(x_new=torch.full((T + 1, dm.n), SENTINEL, dtype=dev.F64, device=device),
             u_new=torch.full((T, dm.m), SENTINEL, dtype=dev.F64, device=device),
             cost=torch.full((1,), SENTINEL, dtype=dev.F64, device=device),
             info=torch.full((3,), INFO_SENTINEL, dtype=torch.int32, device=device))
    s = dict(rho=10.0, relax=1.6, max_iter=5000, eps=1e-8)
    s.update(qp)
    one = [d[k][b] for k in ("xd", "x0", "xlo", "xhi", "ulo", "uhi")]
    assert all(t.is_contiguous() for t in one)
    check(dm.lib.irs_tvlqr_box_descent_if(dm.model_id, dm._p, dm._np, T, d["At"][b].data_ptr(), d["Bt"][b].data_ptr(),
                                          d["ct"][b].data_ptr(), d["Q"].data_ptr(), d["Qd"].data_ptr(), d["R"].data_ptr(),
                                          0.5, *[t.data_ptr() for t in one], s["rho"], s["relax"], s["max_iter"], s["eps"],
                                          o["x_new"].data_ptr(), o["u_new"].data_ptr(), o["cost"].data_ptr(),
                                          o["info"].data_ptr(), None, dev._stream()), "irs_tvlqr_box_descent_if")
    return {k: npy(v) for k, v in o.items()}


def single_wsx(dm, d, b):
    """irs_tvlqr_box_descent_wsx on problem b's blocks, its records forced into a workspace (no cost output)."""
    o = dm.tvlqr_box_descent(d["At"][b], d["Bt"][b], d["ct"][b], d["Q"], d["Qd"], d["R"], d["xd"][b], d["x0"][b],
                             d["xlo"][b], d["xhi"][b], d["ulo"][b], d["uhi"][b], records_in_hbm=True)
    return {k: npy(o[k]) for k in ("x_new", "u_new", "info")}


def prefilled(dm, B, T, device):
    from irs_mpc_amd import device as dev
    return dict(x_new=torch.full((B, T + 1, dm.n), SENTINEL, dtype=dev.F64, device=device),
                u_new=torch.full((B, T, dm.m), SENTINEL, dtype=dev.F64, device=device),
                cost=torch.full((B,), SENTINEL, dtype=dev.F64, device=device),
                info=torch.full((B, 3), INFO_SENTINEL, dtype=torch.int32, device=device))


def batch(dm, d, **kw):
    B, T = d["At"].shape[0], d["At"].shape[1]
    out = prefilled(dm, B, T, d["At"].device)
    dm.tvlqr_box_descent_batch(*[d[k] for k in ARRAYS], out=out, **kw)
    torch.cuda.synchronize()
    return {k: npy(v) for k, v in out.items()}


def shows_something(c, one):
    """The single call converged on every tail and its bound is reached to 1e-6 (and kept)."""
    assert one["info"][0] == 0 and one["info"][2] == 0 and 0 < one["info"][1] < 5000, one["info"]
    key, comp, lo, hi = c["bound"]
    v = one[key][1:, comp] if key == "x_new" else one[key][:, comp]
    assert v.min() >= lo - 1e-6 and v.max() <= hi + 1e-6, (v.min(), v.max())
    assert min(abs(v.min() - lo), abs(v.max() - hi)) <= 1e-6, (v.min(), v.max(), lo, hi)


def equal_to_single(got, b, one, keys=KEYS):
    for key in keys:
        g, w = got[key][b].reshape(-1), one[key].reshape(-1)
        assert np.array_equal(g, w), (b, key, g, w)


# ---------------------------------------------------------------- 1. the kernel against the singles, bit for bit
@pytest.mark.parametrize("name", ["bicycle", "pendulum", "quadrotor"])
@pytest.mark.parametrize("hbm", [False, True], ids=["records-on-chip", "records-in-hbm"])
def test_batch_equals_single_bounded_descents_bit_for_bit(amd, name, hbm):
    """B = 3: x_new, u_new, cost and info[3] of problem b are the bits of irs_tvlqr_box_descent_if on problem b's
    inputs; with the records in HBM (slices at b * stride) also those of irs_tvlqr_box_descent_wsx."""
    c = kernel_case(name)
    dm = device_system(amd, name).dm()
    d = on_device(c)
    singles = [single_if(dm, d, b) for b in range(3)]
    for one in singles:
        shows_something(c, one)
    got = batch(dm, d, records_in_hbm=hbm)
    for b in range(3):
        equal_to_single(got, b, singles[b])
        print(name, "hbm" if hbm else "lds", b, "info", got["info"][b], "max |batch - single| x_new",
              np.abs(got["x_new"][b] - singles[b]["x_new"]).max())
        if hbm:
            equal_to_single(got, b, single_wsx(dm, d, b), keys=("x_new", "u_new", "info"))
    if hbm:
        stride = dm.lib.irs_tvlqr_box_descent_batch_workspace_bytes(dm.model_id, d["At"].shape[1], 1)
        assert stride > 0 and stride % 256 == 0


# ---------------------------------------------------------------- 2. run_flag
def test_run_flag_zero_problems_are_not_touched(amd):
    """Bicycle, B = 4 (problem 3 = problem 0's data), run_flag = [1,0,1,0]: problems 1 and 3 keep the sentinel in every
    output, problems 0 and 2 equal their singles; run_flag = [0,0,0,0]: nothing is written."""
    c = kernel_case("bicycle")
    dm = device_system(amd, "bicycle").dm()
    d = on_device(c, order=(0, 1, 2, 0))
    singles = {b: single_if(dm, d, b) for b in (0, 2)}
    for one in singles.values():
        shows_something(c, one)
    for hbm in (False, True):
        flag = torch.tensor([1, 0, 1, 0], dtype=torch.int32, device=d["At"].device)
        got = batch(dm, d, run_flag=flag, records_in_hbm=hbm)
        for b in (1, 3):
            assert (got["x_new"][b] == SENTINEL).all() and (got["u_new"][b] == SENTINEL).all()
            assert got["cost"][b] == SENTINEL and (got["info"][b] == INFO_SENTINEL).all()
        for b in (0, 2):
            equal_to_single(got, b, singles[b])
        got = batch(dm, d, run_flag=torch.zeros_like(flag), records_in_hbm=hbm)
        assert (got["x_new"] == SENTINEL).all() and (got["u_new"] == SENTINEL).all()
        assert (got["cost"] == SENTINEL).all() and (got["info"] == INFO_SENTINEL).all()


# ---------------------------------------------------------------- 3. a failed neighbour stays alone
def test_non_pd_problem_reports_alone_and_leaves_its_neighbours_bits(amd):
    """The construction of test_descent_batch_equals_single_descents_bit_for_bit (a negative direction in the shared R,
    the last problem's B_{T-1} = 0), moved past the ADMM's own term: the kernel factorises H = alpha R + rho/2 + B'PB on
    a bounded control, so R = -1e-3 is covered for every problem by rho/2 = 5.  The smallest perturbation of that kind
    that leaves a negative direction is R just below -rho / (2 alpha) = -10; R = -10.0002 makes alpha R + rho/2 = -1e-4
    -- the same order as the Riccati test's alpha R = -5e-4 -- which B'PB (>= 2.4e-3 along these trajectories) covers
    for every problem but the last at t = T - 1.  Only that problem's info[0] is non-zero (= T), and the others are the
    bits of their singles built from the same R."""
    c = kernel_case("pendulum")
    dm = device_system(amd, "pendulum").dm()
    T = c["At"].shape[1]
    Bt = c["Bt"].copy()
    Bt[2, T - 1] = 0.0
    d = on_device(c, Bt=Bt, R=np.diag([-10.0002]))
    shows_something(c, single_if(dm, on_device(c), 0))
    for hbm in (False, True):
        got = batch(dm, d, records_in_hbm=hbm)
        for b in range(3):
            one = single_if(dm, d, b)
            assert (one["info"][0] != 0) == (b == 2), (b, one["info"])
            equal_to_single(got, b, one)
            if b != 2:
                assert np.isfinite(got["x_new"][b]).all() and np.isfinite(got["cost"][b])
        assert got["info"][2, 0] == T, got["info"]


# ---------------------------------------------------------------- 4.-6. the class against its twins
def class_problems(amd, qp_max_iter=None):
    """tests/test_irs_lqr_batch_gpu.py's trio: pendulum, T = 10, problem 1 with |u| <= 0.2."""
    from examples.problems import pendulum
    ps, smps = [], []
    for b in range(3):
        system, p, smoothing, _, _ = pendulum(CLS_T)
        p.x0 = np.array([0.1 * b, 0.0])
        p.u_trj_initial = np.tile(np.array([0.1 + 0.02 * b]), (CLS_T, 1))
        if b == BOUND:
            p.ubound = np.array([[-0.2], [0.2]])             # the first descent already asks for more torque
        if qp_max_iter is not None:
            p.qp_max_iter = qp_max_iter
        ps.append(p)
        smps.append(amd.GaussianSmoothing(0.3 * np.ones(2), 0.2 * np.ones(1) * (1 + b), CLS_N, power=smoothing["power"],
                                          seed=40 + b))
    return system, ps, smps


def bicycle_problems(amd):
    ps = []
    for b in range(3):
        p = amd.IrsLqrParameters()
        p.Q, p.Qd, p.R = bike_weights()
        p.x0, p.u_trj_initial, p.xd_trj = starts("bicycle", b)
        p.xbound = [-np.array([np.inf] * 4 + [np.pi / 4]), np.array([np.inf] * 4 + [np.pi / 4])]
        ps.append(p)
    return amd.BicycleDynamics(0.1), ps


def assert_bits_of_twin(batch, b, twin):
    assert np.array_equal(np.array(batch.cost_lst[b]), np.array(twin.cost_lst)), (b, batch.cost_lst[b], twin.cost_lst)
    assert len(batch.x_trj_lst[b]) == len(twin.x_trj_lst)
    for i in range(len(twin.x_trj_lst)):
        assert np.array_equal(batch.x_trj_lst[b][i], twin.x_trj_lst[i]), (b, i)
    assert np.array_equal(batch.x_trj[b], twin.x_trj) and np.array_equal(batch.u_trj[b], twin.u_trj), b


def test_bounded_class_exact_equals_its_twins_bit_for_bit(amd):
    """order "exact", 3 iterations: every problem -- the bound one too -- finishes with status None and the bits of
    IrsLqrExact on the same params (whose fused loop runs the same kernels).  Pendulum trio (one bound problem), then
    the bicycle T = 12 trio (the steer bound binds in all three)."""
    system, ps, _ = class_problems(amd)
    for system, ps, bound in ((system, ps, [BOUND]), bicycle_problems(amd) + ([0, 1, 2],)):
        batch = amd.IrsLqrBatch(system, ps, "exact", bounded=True)
        batch.iterate(CLS_ITERS)
        assert batch.status == [None] * 3, batch.status
        for b in range(3):
            twin = amd.IrsLqrExact(system, ps[b])
            twin.verbose = False
            twin.iterate(CLS_ITERS)
            assert len(batch.cost_lst[b]) == len(twin.cost_lst) == CLS_ITERS + 2
            assert_bits_of_twin(batch, b, twin)
        for b in bound:                     # the first descent's result sits on the bound (the kernel cases above)
            if system.dim_x == 5:
                reached = np.abs(batch.x_trj_lst[b][1][:, 4]).max() - np.pi / 4
            else:
                reached = np.abs(batch.u_trj_lst[b][1]).max() - 0.2
            assert abs(reached) <= 1e-6, (b, reached)
        flags, box_info = npy(batch._last["flag"]), npy(batch._last["box_info"])
        assert box_info.shape == (3, 3) and not box_info[:, 0].any() and not box_info[:, 2].any(), box_info
        assert all((box_info[b, 1] > 0) == (flags[b] != 0) for b in range(3)), (flags, box_info)
        assert batch.iter == CLS_ITERS + 1


@pytest.mark.parametrize("order", ["zero_order", "first_order"])
def test_bounded_class_sampled_orders_against_their_twins(amd, order):
    """N = 2500: batch and twin agree as two loops on f32 statistics do (the existing file's tolerance: rtol 1e-4 on
    cost_lst; trajectories at the same rtol with an atol of 1e-4 of the trajectory's largest entry) -- the bound problem
    too.  The measured ratio is printed."""
    system, ps, smps = class_problems(amd)
    batch = amd.IrsLqrBatch(system, ps, order, smps, bounded=True)
    batch.iterate(CLS_ITERS)
    assert batch.status == [None] * 3, batch.status
    single = {"zero_order": "IrsLqrZeroOrder", "first_order": "IrsLqrFirstOrder"}[order]
    for b in range(3):
        twin = getattr(amd, single)(system, ps[b], smps[b])
        twin.verbose = False
        twin.iterate(CLS_ITERS)
        assert len(batch.cost_lst[b]) == len(twin.cost_lst) == CLS_ITERS + 2
        print(order, b, "cost_lst rel diff", np.abs(np.array(batch.cost_lst[b]) / np.array(twin.cost_lst) - 1).max(),
              "x_trj abs diff", np.abs(batch.x_trj[b] - twin.x_trj).max(), "u_trj abs diff",
              np.abs(batch.u_trj[b] - twin.u_trj).max())
        np.testing.assert_allclose(batch.cost_lst[b], twin.cost_lst, rtol=LOOP_RTOL)
        np.testing.assert_allclose(batch.x_trj[b], twin.x_trj, rtol=LOOP_RTOL, atol=1e-4 * np.abs(twin.x_trj).max())
        np.testing.assert_allclose(batch.u_trj[b], twin.u_trj, rtol=LOOP_RTOL, atol=1e-4 * np.abs(twin.u_trj).max())
    assert np.abs(batch.u_trj[BOUND]).max() <= 0.2 + 1e-12


def test_unsolved_bounded_qp_stops_its_problem_only(amd):
    """qp_max_iter = 3 on all params: the bound problem's tails stop at the limit, its status is the single class's
    message and its trajectory the last adopted one (the initial one); the other two finish as their twins."""
    system, ps, _ = class_problems(amd, qp_max_iter=3)
    batch = amd.IrsLqrBatch(system, ps, "exact", bounded=True)
    x_init, u_init = batch.x_trj.copy(), batch.u_trj.copy()
    batch.iterate(CLS_ITERS)
    assert batch.status[BOUND] == QP_FAILED, batch.status
    assert np.array_equal(batch.x_trj[BOUND], x_init[BOUND]) and np.array_equal(batch.u_trj[BOUND], u_init[BOUND])
    assert len(batch.cost_lst[BOUND]) == 1
    twin = amd.IrsLqrExact(system, ps[BOUND])
    twin.verbose = False
    with pytest.raises(ValueError, match="TV_LQR failed"):
        twin.iterate(CLS_ITERS)
    for b in (0, 2):
        assert batch.status[b] is None, batch.status
        twin = amd.IrsLqrExact(system, ps[b])
        twin.verbose = False
        twin.iterate(CLS_ITERS)
        assert_bits_of_twin(batch, b, twin)


# ---------------------------------------------------------------- 7. constructor refusals
def test_bounded_constructor_refusals(amd):
    system, ps, _ = class_problems(amd)
    ps[2].qp_eps = 1e-6
    with pytest.raises(ValueError, match="qp_eps"):
        amd.IrsLqrBatch(system, ps, "exact", bounded=True)
    system, ps, _ = class_problems(amd)
    ps[0].qp_adaptive_rho = True
    with pytest.raises(NotImplementedError, match="qp_adaptive_rho"):
        amd.IrsLqrBatch(system, ps, "exact", bounded=True)
    # a finite bound beyond the kernel's horizon: the single class's message
    from examples.problems import pendulum
    limit = amd.PendulumDynamics(0.05).dm().box_horizon_limit()
    system, p, _, _, _ = pendulum(limit + 1)
    p.ubound = np.array([[-0.2], [0.2]])
    text = ("a box bound is active and horizon T=%d is beyond the bounded TV-LQR kernel's limit T <= %d "
            "(factor records in HBM, ADMM vectors in LDS; tv_lqr.py:112-123)" % (limit + 1, limit))
    with pytest.raises(NotImplementedError) as e:
        amd.IrsLqrBatch(system, [p], "exact", bounded=True)
    assert str(e.value) == text
    amd.IrsLqrBatch(system, [p], "exact")                     # bounded=False: today's class takes it
