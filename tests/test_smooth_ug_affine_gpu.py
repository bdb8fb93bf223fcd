"""The affine table rows and the tabulated dual-step columns of the uniform-geometry sample pass (csrc/smooth_ug.hip).

A primal-dual iteration and a repair round read  h_A + H_A du  (h_A = G_A r0, H_A = G_A C') instead of applying the 8 x 8
map G_A to r = r0 + C du, and a dual active-set step of the zero-order pass reads its direction u = G_A W[:,p] as a
column of the tabulated U_A = G_A W.  Two views of that:

1. one sample per `sums` row (N = 1): every sample's solve is visible on its own, against the f64 oracle.  A NumPy twin
   of the first attempt (6 sweeps at omega = 1.5, 4 primal-dual iterations, tolerance 1e-6 max|r|) certifies that the
   inputs do go through the new paths: rows that park (repair rounds + dual steps), rows that end on the empty set,
   rows that end with four or more active contacts;
2. several trips and the end-of-pass flush in one workgroup, and two workgroups per time step, both modes, against the
   oracle and the general kernel (IRS_UG=0), bit-equal from run to run.
"""
import os

import numpy as np
import pytest
import torch

from oracle import irs_oracle as orc

pytestmark = pytest.mark.gpu

FP32_TOL = dict(rtol=1e-4, atol=2e-5)       # the project's f32 tolerance of the sample pass (tests/test_gpu_parity.py)
HAND = orc.PlanarHandOracle
HAND_IDX = np.array([1, 4, 2, 5])
SWEEPS, PDAS, OMEGA, PIVOT = 6, 4, 1.5, 1e-5            # csrc/smooth_ug.hip: IRS_UG_SWEEPS, IRS_UG_PDAS, the table's pivot rule
SEED_ROWS = 7                                           # chosen on the CPU: the twin's counts below hold (see the test)
SEED_TRIPS = 11


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return irs_mpc_amd


# ------------------------------------------------------------------------------------------------ the NumPy twin
def dual_problem(sys_o, x, u):
    """W (8,8) and r (8,) of the step QP's dual at one state and command."""
    Dinv, b, J, phi = sys_o._qp(x[None], u[None])
    JD = J[0] * Dinv
    return JD.dot(J[0].T), phi[0] - JD.dot(b[0])


def table_row(W, r, a):
    """What table entry `a` returns: the reduced set (rows of `a` in order, a row whose Schur complement on the rows
    accepted so far is below PIVOT W_ii drops out) and v = [lam on the set ; slacks off it]."""
    nc = len(r)
    S = []
    for j in range(nc):
        if not (a >> j) & 1:
            continue
        d = W[j, j] - (W[j, S].dot(np.linalg.solve(W[np.ix_(S, S)], W[S, j])) if S else 0.0)
        if d > PIVOT * W[j, j]:
            S.append(j)
    lam = np.zeros(nc)
    if S:
        lam[S] = np.linalg.solve(W[np.ix_(S, S)], -r[S])
    on = np.zeros(nc, bool)
    on[S] = True
    return on, np.where(on, lam, r + W.dot(lam))


def bits(mask):
    return int(sum(1 << i for i in range(len(mask)) if mask[i]))


def twin_try(W, r):
    """ug_try in f64: (settled, set).  settled: the set is the optimal one; else the set the iteration stopped on."""
    nc = len(r)
    lam, g = np.zeros(nc), r.copy()
    for _ in range(SWEEPS):
        for i in range(nc):
            nw = max(lam[i] - g[i] * OMEGA / W[i, i], 0.0)
            g += W[:, i] * (nw - lam[i])
            lam[i] = nw
    a = bits(lam > 0)
    tol = 1e-6 * max(np.abs(r).max(), 1e-30)
    for _ in range(PDAS):
        on, v = table_row(W, r, a)
        bad = np.where(on, v, v + tol) < 0
        if not bad.any():
            return True, bits(on)
        a = bits(on) ^ bits(bad)
    return False, a


def twin_counts(sys_o, X, U, du):
    """(parked, ends on the empty set, ends with >= 4 active rows) over the samples du[t, s] of the rows (X[t], U[t])."""
    parked = empty = many = 0
    for t in range(X.shape[0]):
        for s in range(du.shape[1]):
            W, r = dual_problem(sys_o, X[t], U[t] + du[t, s].astype(np.float64))
            settled, a = twin_try(W, r)
            if not settled:
                parked += 1
                a = bits(sys_o._dual_exact(W[None], r[None])[0] > 0)          # where the full method ends
            empty += a == 0
            many += bin(a).count("1") >= 4
    return parked, empty, many


# ------------------------------------------------------------------------------------------------ the inputs
def bench_rows(k):
    """k states of the benchmark's T = 50 rollout (bench.py: the planar hand at rest under its initial command), cycled."""
    sys_o = HAND(0.1)
    x0 = HAND.pack([0.0, 0.35, 0.0], [-np.pi / 4, -np.pi / 4], [np.pi / 4, np.pi / 4])
    u_trj = np.tile(x0[HAND_IDX], (50, 1))
    x_trj = orc.rollout(sys_o, x0, u_trj)
    idx = np.arange(k) % 50
    return x_trj[idx], u_trj[idx]


def random_rows(rng, k):
    """The generator of test_uniform_geometry_kernel_on_random_states: separated, touching, deeply penetrating."""
    obj = np.stack([rng.uniform(-0.3, 0.3, k), rng.uniform(0.1, 0.7, k), rng.uniform(-1, 1, k)], 1)
    left = np.stack([rng.uniform(-2.2, -0.2, k), rng.uniform(-1.5, 0.5, k)], 1)
    right = np.stack([rng.uniform(0.2, 2.2, k), rng.uniform(-0.5, 1.5, k)], 1)
    X = np.zeros((k, 7))
    X[:, HAND.PERM] = np.hstack([obj, left, right])
    U = X[:, HAND_IDX] + rng.normal(0, 0.1, (k, 4))
    return X, U


def one_sample_rows(seed=SEED_ROWS):
    rng = np.random.default_rng(seed)
    Xb, Ub = bench_rows(128)
    Xr, Ur = random_rows(rng, 128)
    du = np.concatenate([0.3 * rng.normal(size=(128, 1, 4)), 0.5 * rng.normal(size=(128, 1, 4))]).astype(np.float32)
    return np.vstack([Xb, Xr]), np.vstack([Ub, Ur]), du


def trip_rows(seed=SEED_TRIPS):
    """Three time steps for the trips test: states 0, 25 and 49 of the benchmark's rollout.  The test is about the control
    flow (trips, flush, two workgroups), and it holds B to FP32_TOL at std 0.02, where a per-sample error of the step is
    divided by the std: with f32 multipliers good to about eps32 |lam| / (smallest pivot of W_AA, relative), the absolute
    tolerance 2e-5 needs |lam| / pivot < 2e-5 * 0.02 / 6e-8 ~ 7.  The grasp of the benchmark has 4.1 (|lam| 3.8, pivot
    0.92); a deeply penetrating random state (|lam| 1600, pivot 0.04) is four orders of magnitude beyond what that
    tolerance can ask of ANY f32 solve at this std -- such states are held per sample in the one-sample-per-row test and at
    N = 1200 in test_uniform_geometry_kernel_on_random_states."""
    X, U = bench_rows(50)
    return X[[0, 25, 49]], U[[0, 25, 49]], np.random.default_rng(seed)


def u_block_of_sums(so, n=7, m=4):
    """The ZERO_ORDER_B layout [Gram of du | du (f - xb)' | sum du] cut out of the oracle's z = [dx | du] layout."""
    d = n + m
    iu = np.triu_indices(d)
    ng = len(iu[0])
    gram = [q for q in range(ng) if iu[0][q] >= n]
    zdf = [ng + i * n + k for i in range(n, d) for k in range(n)]
    sz = [ng + d * n + i for i in range(n, d)]
    return so[:, gram + zdf + sz]


# ------------------------------------------------------------------------------------------------ the tests
def test_one_sample_per_row_vs_oracle(amd):
    """T = 256 rows of ONE sample each through dm.smooth_accumulate(ZERO_ORDER_B): 128 states of the benchmark's rollout
    (std 0.3) and 128 random states (std 0.5), every row against the f64 oracle's sums to FP32_TOL.  By the twin the rows
    exercise the affine lookups of the first attempt, the repair rounds and dual steps of the parked ones (>= 24), the
    empty set (>= 8) and large sets (>= 8 rows with four or more active contacts).
    Measured on an MI355X, max |sums - oracle| over the 256 rows and the largest error in units of the tolerance
    (|err| / (atol + rtol |oracle|)): 3.046e-4 and 0.95 with the affine rows, 3.050e-4 and 0.67 with the direct rows they
    replaced (the benchmark's rows alone: 2.1e-6 and 0.07 against 3.1e-6 and 0.12) -- both inside FP32_TOL, so that is the bound."""
    from irs_mpc_amd import device as dev
    from irs_mpc_amd._lib import SMOOTH_ZERO_ORDER_B
    sys_o = HAND(0.1)
    X, U, du = one_sample_rows()
    parked, empty, many = twin_counts(sys_o, X, U, du)
    print("twin: %d of 256 rows park, %d end on the empty set, %d with >= 4 active rows" % (parked, empty, many))
    assert parked >= 24 and empty >= 8 and many >= 8
    so = u_block_of_sums(orc.zero_order_sums(sys_o, X, U, np.zeros((256, 1, 7)), du.astype(np.float64), sum_z=True))
    dm = amd.PlanarHandDynamics(0.1).dm()
    sums = dm.smooth_accumulate(SMOOTH_ZERO_ORDER_B, dev.to_dev(X), dev.to_dev(U), None, dev.to_dev(du, dev.F32))
    got = sums.cpu().numpy()
    assert got.shape == so.shape == (256, 42)
    err = np.abs(got - so)
    print("one sample per row: max |sums - oracle| %.3e, max of |err| / (atol + rtol |oracle|) %.3f" % (
        err.max(), (err / (FP32_TOL["atol"] + FP32_TOL["rtol"] * np.abs(so))).max()))
    np.testing.assert_allclose(got, so, **FP32_TOL)


@pytest.mark.parametrize("N", [200, 700], ids=["one_workgroup", "two_workgroups"])
def test_trips_and_flush_vs_oracle_and_general_kernel(amd, N):
    """T = 3, N = 200 (four trips of one wave's share and the end-of-pass flush inside ONE workgroup) and N = 700 (two
    workgroups per time step), std 0.02 and 0.5, both modes: against the oracle and the general kernel (IRS_UG=0) to the
    tolerances of test_uniform_geometry_kernel_on_random_states, info == 0, and a second run bit-equal."""
    from irs_mpc_amd import device as dev
    from irs_mpc_amd._lib import SMOOTH_FIRST_ORDER, SMOOTH_ZERO_ORDER_B
    sys_o = HAND(0.1)
    X, U, rng = trip_rows()
    xp = np.vstack([X, X[-1:]])
    dm = amd.PlanarHandDynamics(0.1).dm()
    xd, ud = dev.to_dev(X), dev.to_dev(U)
    for std in (0.02, 0.5):
        du = (std * rng.normal(size=(3, N, 4))).astype(np.float32)
        if N == 200 and std == 0.5:
            parked = twin_counts(sys_o, X, U, du[:, :64])[0]
            print("twin: %d of the first 3 x 64 samples park" % parked)
            assert parked >= 3                      # the flush has something to do
        dud = dev.to_dev(du, dev.F32)
        for mode in (SMOOTH_ZERO_ORDER_B, SMOOTH_FIRST_ORDER):
            outs = {}
            for ug in ("1", "0"):
                os.environ["IRS_UG"] = ug
                try:
                    o = dm.smooth(mode, xd, ud, None, dud)
                    outs[ug] = {kk: o[kk].cpu().numpy() for kk in ("At", "Bt", "ct", "info")}
                finally:
                    os.environ.pop("IRS_UG", None)
            assert int(np.abs(outs["1"]["info"]).sum()) == 0
            np.testing.assert_array_equal(outs["1"]["At"], outs["0"]["At"])
            if mode == SMOOTH_ZERO_ORDER_B:
                _, Bo, co = orc.zero_order_B_decoupled(sys_o, xp, U, du.astype(np.float64))
                print("N %d std %.2f zero-order-B: |B - oracle| %.2e |c - oracle| %.2e |B - general| %.2e" % (
                    N, std, np.abs(outs["1"]["Bt"] - Bo).max(), np.abs(outs["1"]["ct"] - co).max(),
                    np.abs(outs["1"]["Bt"] - outs["0"]["Bt"]).max()))
                np.testing.assert_allclose(outs["1"]["Bt"], outs["0"]["Bt"], **FP32_TOL)
                np.testing.assert_allclose(outs["1"]["ct"], outs["0"]["ct"], **FP32_TOL)
                np.testing.assert_allclose(outs["1"]["Bt"], Bo, **FP32_TOL)
                np.testing.assert_allclose(outs["1"]["ct"], co, **FP32_TOL)
            else:
                _, Bo, _ = orc.first_order_B_decoupled(sys_o, xp, U, du.astype(np.float64))
                print("N %d std %.2f first-order: |B - oracle| %.2e |B - general| %.2e (bound %.2e)" % (
                    N, std, np.abs(outs["1"]["Bt"] - Bo).max(), np.abs(outs["1"]["Bt"] - outs["0"]["Bt"]).max(), 20.0 / N))
                # piecewise constant in the sample: two f32 routes may put a borderline sample on different faces
                assert np.abs(outs["1"]["Bt"] - outs["0"]["Bt"]).max() < 20.0 / N
                assert np.abs(outs["1"]["Bt"] - Bo).max() < 20.0 / N
            o2 = dm.smooth(mode, xd, ud, None, dud)
            assert np.array_equal(o2["Bt"].cpu().numpy(), outs["1"]["Bt"])
            assert np.array_equal(o2["ct"].cpu().numpy(), outs["1"]["ct"])
