"""Batched iRS-LQR for the analytic models on the device: irs_tvlqr_descent_batch bit for bit against B single descents
on every Riccati path, irs_tvlqr_plan_within_bounds_batch against the single entry's decisions,
irs_smooth_rng_general_batch against the f64 oracle on identical samples (at the single entry's tolerance, and no wider
than its single twin gets), and IrsLqrBatch against B runs of the single classes."""
import functools

import numpy as np
import pytest
import torch

from oracle import irs_oracle as orc
from oracle import tvlqr_highprec as hp

pytestmark = pytest.mark.gpu

ZERO_ORDER_AB, FIRST_ORDER = 0, 1
# tests/test_gpu_parity.py:23 -- the stated fp32 tolerance of the sample pass against the f64 oracle on identical samples
FP32_TOL = dict(rtol=1e-4, atol=2e-5)
# tests/test_gpu_parity.py:364-366 -- test_mode_G_smoothing_vs_oracle, the single entry's device-RNG test of the pendulum
# in zero order and of the quadrotor in first order
MODE_G_TOL = dict(rtol=2e-4, atol=5e-5)
# tests/test_gpu_parity.py:515 -- two loops on f32 statistics: rtol on cost_lst
LOOP_RTOL = 1e-4


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
            "bicycle": amd.BicycleDynamics(0.1), "three_cart": amd.ThreeCartDynamics(0.05)}[name]


# ---------------------------------------------------------------- the descent, bit for bit
def random_problems(n, m, T, B, seed):
    """A_t = I + 0.1 N(0,1), B_t standard normal, c_t = 0.1 N(0,1) (oracle/tvlqr_highprec.py, riccati_problem), with a
    start state and a goal trajectory of its own per problem."""
    rng = np.random.default_rng([n, m, T, B, seed])
    return dict(At=np.eye(n) + 0.1 * rng.normal(size=(B, T, n, n)), Bt=rng.normal(size=(B, T, n, m)),
                ct=0.1 * rng.normal(size=(B, T, n)), xd=rng.normal(size=(B, T + 1, n)), x0=0.3 * rng.normal(size=(B, n)))


def model_problems(name, h, T, B):
    """The exact linearisation along the example's rollout (oracle/tvlqr_highprec.py, model_problem: the closed loop
    on the true dynamics stays finite at any horizon), the start state and the goal shifted per problem."""
    p = hp.model_problem(name, h, T)
    rng = np.random.default_rng([T, B])
    n = p["x0"].shape[0]
    return dict(At=np.stack([p["At"]] * B), Bt=np.stack([p["Bt"]] * B), ct=np.stack([p["ct"]] * B),
                xd=np.stack([p["xd"] + 0.01 * rng.normal(size=n) for _ in range(B)]),
                x0=np.stack([p["x0"] + 0.01 * rng.normal(size=n) for _ in range(B)]))


DESCENT_CASES = [("pendulum", 3, 5, "registers"), ("quadrotor", 3, 4, "matrix-core"), ("three_cart", 2, 4, "matrix-core"),
                 ("quadrotor", 2, 341, "lds"), ("quadrotor", 1, 341, "lds")]


@pytest.mark.parametrize("name,B,T,path", DESCENT_CASES, ids=["%s-B%d-T%d-%s" % c for c in DESCENT_CASES])
def test_descent_batch_equals_single_descents_bit_for_bit(amd, name, B, T, path):
    """K, k, x_new, u_new, cost and info of problem b are the bits of irs_tvlqr_descent on problem b's inputs.
    Q, Qd and R are shared by the problems of a launch, so `its own non-positive-definite R` is built from the shared
    one: R has a negative direction, which B'PB covers for every problem but the last, whose B_{T-1} is zero -- its
    H = alpha R + B'PB alone is not positive definite, only its info is non-zero, and the neighbours still equal their
    single descents."""
    from irs_mpc_amd import device as dev
    system = device_system(amd, name)
    dm = system.dm()
    n, m = system.dim_x, system.dim_u
    p = model_problems(name, 0.05, T, B) if T > 100 else random_problems(n, m, T, B, 0)
    rng = np.random.default_rng([n, m, T])
    Q, Qd = np.diag(rng.uniform(0.5, 2.0, n)), np.diag(rng.uniform(5.0, 20.0, n))
    R = np.diag(rng.uniform(0.5, 2.0, m))
    bad = B - 1 if B > 1 else None
    if bad is not None:
        R[0, 0] = -1e-3
        p["Bt"][bad, T - 1] = 0.0
    d = {k: dev.to_dev(v) for k, v in p.items()}
    Qd_, Q_, R_ = dev.to_dev(Qd), dev.to_dev(Q), dev.to_dev(R)
    got = dm.tvlqr_descent_batch(d["At"], d["Bt"], d["ct"], Q_, Qd_, R_, d["xd"], d["x0"])
    torch.cuda.synchronize()
    for b in range(B):
        one = dm.tvlqr_descent(d["At"][b], d["Bt"][b], d["ct"][b], Q_, Qd_, R_, d["xd"][b], d["x0"][b].contiguous())
        for key in ("K", "k", "x_new", "u_new", "cost", "info"):
            g, w = npy(got[key][b]).reshape(-1), npy(one[key]).reshape(-1)
            assert np.array_equal(g, w, equal_nan=True), (name, T, b, key, np.abs(g - w).max())
        info = int(npy(got["info"])[b])
        assert (info != 0) == (b == bad), (b, info)
        if b != bad:
            assert np.isfinite(npy(got["x_new"][b])).all() and np.isfinite(npy(got["cost"][b]))


# ---------------------------------------------------------------- the plan test
def test_plan_within_bounds_batch_equals_the_single_entry(amd):
    """B = 4 pendulum problems, T = 5, a box each: two that never bind (+-1e4, +-inf), one cut on u just inside the
    realised max |u|, one cut on x.  flag[b] is the single entry's decision on problem b."""
    from irs_mpc_amd import device as dev
    system = device_system(amd, "pendulum")
    dm = system.dm()
    B, T, n, m = 4, 5, 2, 1
    rng = np.random.default_rng(11)
    x0 = np.stack([[0.2 * b, 0.1] for b in range(B)])
    u0 = 0.1 + 0.05 * rng.normal(size=(B, T, m))
    so = orc.PendulumOracle(0.05)
    X = np.stack([orc.rollout(so, x0[b], u0[b]) for b in range(B)])
    lin = [np.stack(a) for a in zip(*[orc.exact_TV(so, X[b], u0[b]) for b in range(B)])]
    At, Bt, ct = (dev.to_dev(a) for a in lin)
    Q, Qd, R = dev.to_dev(np.diag([1., 1.])), dev.to_dev(np.diag([20., 20.])), dev.to_dev(np.diag([1.]))
    xd = dev.to_dev(np.tile(np.array([np.pi, 0.]), (B, T + 1, 1)))
    o = dm.tvlqr_descent_batch(At, Bt, ct, Q, Qd, R, xd, dev.to_dev(x0))
    u_new, x_new = npy(o["u_new"]), npy(o["x_new"])
    inf = np.inf
    xlo, xhi = np.full((B, n), -inf), np.full((B, n), inf)
    ulo, uhi = np.full((B, m), -inf), np.full((B, m), inf)
    xlo[0], xhi[0], ulo[0], uhi[0] = -1e4, 1e4, -1e4, 1e4
    umax = np.abs(u_new[2]).max()                            # tail t's first control is the realised u_t
    ulo[2], uhi[2] = -0.999 * umax, 0.999 * umax
    xmax = np.abs(x_new[3, 1:, 1]).max()
    xlo[3, 1], xhi[3, 1] = -0.5 * xmax, 0.5 * xmax
    box = [dev.to_dev(a) for a in (xlo, xhi, ulo, uhi)]
    flag = npy(dm.plan_within_bounds_batch(At, Bt, ct, o["K"], o["k"], o["x_new"], *box))
    one = torch.full((1,), -1, dtype=torch.int32, device=At.device)
    for b in range(B):
        from irs_mpc_amd._lib import check
        check(dm.lib.irs_tvlqr_plan_within_bounds(n, m, T, At[b].data_ptr(), Bt[b].data_ptr(), ct[b].data_ptr(),
                                                  o["K"][b].data_ptr(), o["k"][b].data_ptr(), o["x_new"][b].data_ptr(),
                                                  box[0][b].data_ptr(), box[1][b].data_ptr(), box[2][b].data_ptr(),
                                                  box[3][b].data_ptr(), one.data_ptr(), dev._stream()),
              "irs_tvlqr_plan_within_bounds")
        assert int(one.item()) == int(flag[b]), (b, int(one.item()), flag)
    assert flag.tolist() == [0, 0, 1, 1], flag


# ---------------------------------------------------------------- the sample pass
SMOOTH_CASES = [("pendulum", ZERO_ORDER_AB, MODE_G_TOL, True), ("quadrotor", ZERO_ORDER_AB, FP32_TOL, False),
                ("quadrotor", FIRST_ORDER, MODE_G_TOL, True), ("bicycle", ZERO_ORDER_AB, FP32_TOL, False)]
SMOOTH_T, SMOOTH_N, SMOOTH_B, SMOOTH_IT = 3, 2500, 3, 2
_START = {"pendulum": ([0.0, 0.0], [0.1]), "bicycle": ([0.0, 0.0, 0.1, 1.0, 0.05], [0.1, 0.0]), "quadrotor": ([0.0] * 12, [2.0] * 4)}


@functools.lru_cache(maxsize=None)
def smooth_problem(name):
    """B nominal trajectories, seeds and standard deviations of one model -- and nothing of the device."""
    so = orc.SYSTEMS[name](0.1 if name == "bicycle" else 0.05)
    n, m = so.dim_x, so.dim_u
    rng = np.random.default_rng([sorted(orc.SYSTEMS).index(name), 5])
    x0, u0 = (np.array(v, float) for v in _START[name])
    U = np.stack([np.tile(u0, (SMOOTH_T, 1)) + 0.02 * rng.normal(size=(SMOOTH_T, m)) for _ in range(SMOOTH_B)])
    X = np.stack([orc.rollout(so, x0 + 0.02 * rng.normal(size=n), U[b]) for b in range(SMOOTH_B)])
    std_x = np.stack([(0.1 + 0.05 * b) * np.linspace(1.0, 1.5, n) for b in range(SMOOTH_B)])
    std_u = np.stack([(0.2 - 0.04 * b) * np.linspace(1.0, 0.8, m) for b in range(SMOOTH_B)])
    seeds = [0x123456789ABC + 1000003 * b for b in range(SMOOTH_B)]
    return so, X, U, std_x, std_u, seeds


@functools.lru_cache(maxsize=None)
def smooth_reference(name, mode):
    """The f64 oracle's get_TV_matrices on problem b's own draws (dm.rng_samples), computed once per (model, mode)."""
    import irs_mpc_amd as amd
    so, X, U, std_x, std_u, seeds = smooth_problem(name)
    dm = device_system(amd, name).dm()
    fn = orc.zero_order_TV if mode == ZERO_ORDER_AB else orc.first_order_TV
    out = []
    for b in range(SMOOTH_B):
        dx, du = dm.rng_samples(SMOOTH_T, SMOOTH_N, std_x[b], std_u[b], seeds[b], SMOOTH_IT)
        out.append(fn(so, X[b], U[b], npy(dx).astype(np.float64), npy(du).astype(np.float64)))
    return out


@pytest.mark.parametrize("name,mode,tol,whole_trajectory", SMOOTH_CASES,
                         ids=["%s-mode%d-%s" % (c[0], c[1], "x_stride_T+1" if c[3] else "x_stride_T") for c in SMOOTH_CASES])
def test_general_batch_sample_pass_vs_oracle_and_single_twin(amd, name, mode, tol, whole_trajectory):
    """T = 3, N = 2500: three 256-thread workgroups per row, the last one partial.  The batch and the single twin are
    each held to the oracle on identical samples at the tolerance of the single entry's device-RNG test (the batch gets
    no wider one); the arrival counters are zero again after the call; a second call on the same workspace returns the
    same bits.  max |batch - single| is printed (DESIGN.md 7.1 records it): a finding, not a threshold."""
    from irs_mpc_amd import device as dev
    so, X, U, std_x, std_u, seeds = smooth_problem(name)
    system = device_system(amd, name)
    dm = system.dm()
    T, N, B, n, m = SMOOTH_T, SMOOTH_N, SMOOTH_B, so.dim_x, so.dim_u
    geo = dm.smooth_geometry(mode, T, N, rng=True)
    assert geo["nblk"] >= 2 and geo["block"] == 256 and N % geo["chunk"] != 0, geo
    Xd = dev.to_dev(X) if whole_trajectory else dev.to_dev(X[:, :T])
    assert Xd.stride(0) == ((T + 1) * n if whole_trajectory else T * n)
    Ud = dev.to_dev(U)
    sx, su = dev.to_dev(std_x), dev.to_dev(std_u)
    seed_dev = torch.as_tensor(np.array(seeds, dtype=np.uint64).view(np.int64)).to(Ud.device)
    got = dm.smooth_rng_general_batch(mode, Xd, Ud, N, sx, su, seed_dev, SMOOTH_IT)
    first = {k: npy(v).copy() for k, v in got.items()}
    # every arrival counter of every slice is zero again
    ws = dm._ws[(("smooth_general_batch", mode, T, N), Ud.device)]
    stride = dm.lib.irs_smooth_general_batch_workspace_bytes(dm.model_id, mode, T, N, 1)
    words = npy(ws.view(torch.int32))
    for b in range(B):
        assert not words[b * stride // 4: b * stride // 4 + 1024].any(), b
    again = dm.smooth_rng_general_batch(mode, Xd, Ud, N, sx, su, seed_dev, SMOOTH_IT)
    for k in first:
        assert np.array_equal(first[k], npy(again[k])), k
    assert not first["info"].any()
    ref = smooth_reference(name, mode)
    worst = 0.0
    for b in range(B):
        one = dm.smooth_rng(mode, dev.to_dev(X[b]), dev.to_dev(U[b]), N, std_x[b], std_u[b], seeds[b], SMOOTH_IT)
        assert not npy(one["info"]).any()
        for key, want in zip(("At", "Bt", "ct"), ref[b]):
            single, batch = npy(one[key]), first[key][b]
            worst = max(worst, float(np.abs(batch - single).max()))
            print("%s mode %d problem %d %s: |single - oracle| %.3g, |batch - oracle| %.3g, |batch - single| %.3g"
                  % (name, mode, b, key, np.abs(single - want).max(), np.abs(batch - want).max(),
                     np.abs(batch - single).max()))
            np.testing.assert_allclose(single, want, **tol)
            np.testing.assert_allclose(batch, want, **tol)
        print("%s mode %d problem %d sums: |batch - single| %.3g (bits equal: %s)"
              % (name, mode, b, np.abs(first["sums"][b] - npy(one["sums"])).max(),
                 np.array_equal(first["sums"][b], npy(one["sums"]))))
    print("%s mode %d: max |batch - single| over At, Bt, ct = %.3g" % (name, mode, worst))


def test_general_batch_rank_deficient_problem_reports_in_its_rows_only(amd):
    """A problem whose standard deviations are zero has a zero Gram matrix: info != 0 in its T rows, 0 in the others'."""
    from irs_mpc_amd import device as dev
    so, X, U, std_x, std_u, seeds = smooth_problem("pendulum")
    dm = device_system(amd, "pendulum").dm()
    std_x, std_u = std_x.copy(), std_u.copy()
    std_x[1], std_u[1] = 0.0, 0.0
    Ud = dev.to_dev(U)
    seed_dev = torch.as_tensor(np.array(seeds, dtype=np.uint64).view(np.int64)).to(Ud.device)
    got = dm.smooth_rng_general_batch(ZERO_ORDER_AB, dev.to_dev(X), Ud, SMOOTH_N, dev.to_dev(std_x), dev.to_dev(std_u),
                                      seed_dev, SMOOTH_IT)
    info = npy(got["info"])
    assert (info[1] != 0).all() and not info[0].any() and not info[2].any(), info
    ref = smooth_reference("pendulum", ZERO_ORDER_AB)
    for b in (0, 2):
        for key, want in zip(("At", "Bt", "ct"), ref[b]):
            np.testing.assert_allclose(npy(got[key])[b], want, **MODE_G_TOL)


# ---------------------------------------------------------------- the class against its twins
CLS_T, CLS_N, CLS_ITERS, BOUND = 10, 2500, 3, 1


def class_problems(amd):
    from examples.problems import pendulum
    ps, smps = [], []
    for b in range(3):
        system, p, smoothing, _, _ = pendulum(CLS_T)
        p.x0 = np.array([0.1 * b, 0.0])
        p.u_trj_initial = np.tile(np.array([0.1 + 0.02 * b]), (CLS_T, 1))
        if b == BOUND:
            p.ubound = np.array([[-0.2], [0.2]])             # the first descent already asks for more torque
        ps.append(p)
        smps.append(amd.GaussianSmoothing(0.3 * np.ones(2), 0.2 * np.ones(1) * (1 + b), CLS_N, power=smoothing["power"],
                                          seed=40 + b))
    return system, ps, smps


@pytest.mark.parametrize("order", ["exact", "zero_order", "first_order"])
def test_irs_lqr_batch_against_its_single_twins(amd, order):
    """B = 3 pendulum problems, T = 10, N = 2500, 3 iterations.  exact: cost_lst, x_trj and u_trj per problem are the
    bits of IrsLqrExact; sampled orders: they agree as two loops on f32 statistics do (rtol 1e-4 on cost_lst,
    tests/test_gpu_parity.py:515; the trajectories at the same rtol, with an atol of 1e-4 of the trajectory's largest
    entry, since angles and speeds cross zero).  Problem 1's u-bound binds at the first descent: its status says so, its
    trajectory stays the initial one, and the other two finish."""
    system, ps, smps = class_problems(amd)
    exact = order == "exact"
    batch = amd.IrsLqrBatch(system, ps, order, None if exact else smps)
    x_init, u_init = batch.x_trj.copy(), batch.u_trj.copy()
    batch.iterate(CLS_ITERS)
    assert batch.status[BOUND] is not None and "box bound is active" in batch.status[BOUND], batch.status
    single = {"exact": "IrsLqrExact", "zero_order": "IrsLqrZeroOrder", "first_order": "IrsLqrFirstOrder"}[order]
    assert single in batch.status[BOUND]
    assert np.array_equal(batch.x_trj[BOUND], x_init[BOUND]) and np.array_equal(batch.u_trj[BOUND], u_init[BOUND])
    assert len(batch.cost_lst[BOUND]) == 1
    for b in (0, 2):
        assert batch.status[b] is None, batch.status
        twin = getattr(amd, single)(system, ps[b]) if exact else getattr(amd, single)(system, ps[b], smps[b])
        twin.verbose = False
        twin.iterate(CLS_ITERS)
        assert len(batch.cost_lst[b]) == len(twin.cost_lst) == CLS_ITERS + 2
        if exact:
            assert np.array_equal(np.array(batch.cost_lst[b]), np.array(twin.cost_lst)), (batch.cost_lst[b], twin.cost_lst)
            assert np.array_equal(batch.x_trj[b], twin.x_trj) and np.array_equal(batch.u_trj[b], twin.u_trj)
            for i in range(len(twin.x_trj_lst)):
                assert np.array_equal(batch.x_trj_lst[b][i], twin.x_trj_lst[i]), i
        else:
            print(order, b, "cost_lst rel diff", np.abs(np.array(batch.cost_lst[b]) / np.array(twin.cost_lst) - 1).max())
            np.testing.assert_allclose(batch.cost_lst[b], twin.cost_lst, rtol=LOOP_RTOL)
            np.testing.assert_allclose(batch.x_trj[b], twin.x_trj, rtol=LOOP_RTOL, atol=1e-4 * np.abs(twin.x_trj).max())
            np.testing.assert_allclose(batch.u_trj[b], twin.u_trj, rtol=LOOP_RTOL, atol=1e-4 * np.abs(twin.u_trj).max())
        assert batch.cost[b] == batch.cost_lst[b][-2]
    assert batch.iter == CLS_ITERS + 1
