"""The single-release primal-dual iteration of the uniform-geometry sample pass (csrc/smooth_ug.hip, ug_pdas) and the
iterations the flush runs from a parked set before the dual steps, on the device:

(a) one sample per `sums` row, so that every solve is visible on its own, against the f64 oracle: the benchmark's states,
    random states, and the rows of tests/golden/ug_release_hard.npz, which the twin (tests/helpers/ug_release_twin.py)
    sends through the flush's iterations and through the dual steps (tests/test_smooth_ug_release_cpu.py holds that);
(b) several trips and the end-of-pass flush in one workgroup, and two workgroups per time step, both modes, against the
    oracle, info == 0, bit-equal from run to run;
(c) the batched launch bit-equal to solo calls at a size where the flush's iterations run.
"""
import os

import numpy as np
import pytest
import torch

from oracle import irs_oracle as orc
from tests.helpers import ug_release_twin as tw

pytestmark = pytest.mark.gpu

FP32_TOL = dict(rtol=1e-4, atol=2e-5)       # the project's f32 tolerance of the sample pass (tests/test_gpu_parity.py)
HAND = orc.PlanarHandOracle
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "ug_release_hard.npz")
SEED_ROWS, SEED_TRIPS = 7, 23               # SEED_ROWS: the rows of test_smooth_ug_affine_gpu.py's one-sample test
KEYS = ("sums", "At", "Bt", "ct", "info")


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return irs_mpc_amd


def u_block_of_sums(so, n=7, m=4):
    """The ZERO_ORDER_B layout [Gram of du | du (f - xb)' | sum du] cut out of the oracle's z = [dx | du] layout."""
    d = n + m
    iu = np.triu_indices(d)
    ng = len(iu[0])
    gram = [q for q in range(ng) if iu[0][q] >= n]
    zdf = [ng + i * n + k for i in range(n, d) for k in range(n)]
    sz = [ng + d * n + i for i in range(n, d)]
    return so[:, gram + zdf + sz]


def one_sample_rows():
    """128 states of the benchmark's rollout (cycled) at std 0.3, 64 random states at std 0.5 -- the generator, seed and
    draw order of test_smooth_ug_affine_gpu.py's one-sample test, whose first 128 + 64 rows these are -- and the fixture."""
    rng = np.random.default_rng(SEED_ROWS)
    _, x_trj, u_trj = tw.bench_rollout(orc)
    idx = np.arange(128) % 50
    Xr, Ur = tw.random_states(HAND, rng, 128)
    du = np.concatenate([0.3 * rng.normal(size=(128, 1, 4)), 0.5 * rng.normal(size=(128, 1, 4))[:64]]).astype(np.float32)
    f = np.load(FIXTURE)
    return (np.vstack([x_trj[idx], Xr[:64], f["x"]]), np.vstack([u_trj[idx], Ur[:64], f["u"]]),
            np.concatenate([du, f["du"][:, None, :].astype(np.float32)]))


def test_one_sample_per_row_vs_oracle(amd):
    """ZERO_ORDER_B through dm.smooth_accumulate with N = 1, every row against the f64 oracle's sums to FP32_TOL."""
    from irs_mpc_amd import device as dev
    from irs_mpc_amd._lib import SMOOTH_ZERO_ORDER_B
    sys_o = HAND(0.1)
    X, U, du = one_sample_rows()
    T = X.shape[0]
    so = u_block_of_sums(orc.zero_order_sums(sys_o, X, U, np.zeros((T, 1, 7)), du.astype(np.float64), sum_z=True))
    dm = amd.PlanarHandDynamics(0.1).dm()
    got = dm.smooth_accumulate(SMOOTH_ZERO_ORDER_B, dev.to_dev(X), dev.to_dev(U), None, dev.to_dev(du, dev.F32)).cpu().numpy()
    assert got.shape == so.shape == (T, 42)
    unit = np.abs(got - so) / (FP32_TOL["atol"] + FP32_TOL["rtol"] * np.abs(so))
    print("one sample per row (%d rows): max |sums - oracle| %.3e; worst error in units of the tolerance: %.3f "
          "(benchmark rows %.3f, random rows %.3f, fixture rows %.3f)" % (
              T, np.abs(got - so).max(), unit.max(), unit[:128].max(), unit[128:192].max(), unit[192:].max()))
    np.testing.assert_allclose(got, so, **FP32_TOL)


@pytest.mark.parametrize("N", [200, 700], ids=["one_workgroup", "two_workgroups"])
def test_trips_and_flush_vs_oracle(amd, N):
    """T = 3 (states 0, 25 and 49 of the benchmark's rollout), std 0.3, N = 200 (the trips of one wave's share and the
    end-of-pass flush inside ONE workgroup) and N = 700 (two workgroups per time step), both modes: zero-order B and c to
    FP32_TOL and first-order B to 20 / N against the oracle, info == 0, a second run bit-equal."""
    from irs_mpc_amd import device as dev
    from irs_mpc_amd._lib import SMOOTH_FIRST_ORDER, SMOOTH_ZERO_ORDER_B
    sys_o, x_trj, u_trj = tw.bench_rollout(orc)
    X, U = x_trj[[0, 25, 49]], u_trj[[0, 25, 49]]
    xp = np.vstack([X, X[-1:]])
    du = (0.3 * np.random.default_rng(SEED_TRIPS).normal(size=(3, N, 4))).astype(np.float32)
    parked = sum((tw.classify(*tw.dual_problems(sys_o, X[t], U[t], du[t, :64].astype(np.float64)), flush=0)[0] == 0).sum()
                 for t in range(3))
    print("twin: %d of the first 3 x 64 samples park" % parked)
    assert parked >= 3                                    # the flush has something to do
    dm = amd.PlanarHandDynamics(0.1).dm()
    xd, ud, dud = dev.to_dev(X), dev.to_dev(U), dev.to_dev(du, dev.F32)
    g = dm.smooth_geometry(SMOOTH_ZERO_ORDER_B, 3, N)
    assert g["family"] == "uniform_geometry" and g["nblk"] == (1 if N == 200 else 2)
    for mode in (SMOOTH_ZERO_ORDER_B, SMOOTH_FIRST_ORDER):
        o = dm.smooth(mode, xd, ud, None, dud)
        out = {k: o[k].cpu().numpy() for k in ("Bt", "ct", "info")}
        assert int(np.abs(out["info"]).sum()) == 0
        if mode == SMOOTH_ZERO_ORDER_B:
            _, Bo, co = orc.zero_order_B_decoupled(sys_o, xp, U, du.astype(np.float64))
            print("N %d zero-order-B: |B - oracle| %.2e |c - oracle| %.2e" % (
                N, np.abs(out["Bt"] - Bo).max(), np.abs(out["ct"] - co).max()))
            np.testing.assert_allclose(out["Bt"], Bo, **FP32_TOL)
            np.testing.assert_allclose(out["ct"], co, **FP32_TOL)
        else:
            _, Bo, _ = orc.first_order_B_decoupled(sys_o, xp, U, du.astype(np.float64))
            print("N %d first-order: |B - oracle| %.2e (bound %.2e)" % (N, np.abs(out["Bt"] - Bo).max(), 20.0 / N))
            # piecewise constant in the sample: f32 may put a borderline sample on another face than f64
            assert np.abs(out["Bt"] - Bo).max() < 20.0 / N
        o2 = dm.smooth(mode, xd, ud, None, dud)
        assert np.array_equal(o2["Bt"].cpu().numpy(), out["Bt"])
        assert np.array_equal(o2["ct"].cpu().numpy(), out["ct"])


@pytest.mark.parametrize("mode_name", ["zero_order_B", "first_order"])
def test_batched_launch_equals_solo_calls(amd, mode_name):
    """B = 3 problems (three states of the benchmark's rollout each, distinct seeds) at T = 3, N = 700, std 0.3: the
    batched launch bit-equal to three dm.smooth_rng calls."""
    from irs_mpc_amd import device as dev
    from irs_mpc_amd._lib import SMOOTH_FIRST_ORDER, SMOOTH_ZERO_ORDER_B
    mode = SMOOTH_ZERO_ORDER_B if mode_name == "zero_order_B" else SMOOTH_FIRST_ORDER
    _, x_trj, u_trj = tw.bench_rollout(orc)
    rows = np.array([[0, 25, 49, 49], [5, 30, 45, 45], [10, 20, 40, 40]])
    X, U = dev.to_dev(x_trj[rows]), dev.to_dev(u_trj[rows[:, :3]])
    std, seeds, N = np.full((3, 4), 0.3), [3, 1003, 2003 | (1 << 63)], 700
    dm = amd.PlanarHandDynamics(0.1).dm()
    assert dm.smooth_geometry(mode, 3, N, rng=True)["family"] == "uniform_geometry"
    solo = []
    for b in range(3):
        o = dm.smooth_rng(mode, X[b], U[b], N, None, list(std[b]), seeds[b], 1)
        solo.append({k: o[k].clone() for k in KEYS})
    assert all(not bool((s["info"] != 0).any().item()) for s in solo)
    assert not torch.equal(solo[0]["Bt"], solo[1]["Bt"])
    got = dm.smooth_rng_batch(mode, X, U, N, dev.to_dev(std),
                              torch.as_tensor(np.array(seeds, dtype=np.uint64).view(np.int64)).cuda(), 1)
    for k in KEYS:
        assert torch.equal(got[k], torch.stack([s[k] for s in solo])), k
