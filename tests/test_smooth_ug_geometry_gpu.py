"""The lane-parallel geometry of the uniform-geometry sample pass (csrc/ug_geometry.hpp, used by csrc/smooth_ug.hip) and
the first block's perturbations requested from inside the prologue.

1. Same bits.  The geometry is meant to be, element for element, what PlanarHandModel::assemble gives.  The golden file
   tests/golden/ug_geometry_parent.npz was written by the library of the commit before the change, on an MI355X, with
   `states()` below: per state and mode, entry 0 of the table irs_debug_ug_table returns -- [r0 | C | tau | set | W], all
   the sample loop takes from the geometry -- and a SHA-256 of the whole 256 x 116 table.
2. Small shapes: T = 2, N in {1, 64, 65, 600}, both modes, supplied and drawn samples, against the general kernel
   (IRS_UG=0) and the oracle; bit-equal from run to run; one solo-versus-batch check.  N = 1 and N = 65 are where the
   early request can go wrong: waves without a first block, and the clamped last row.
"""
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

from oracle import irs_oracle as orc
from tests.helpers import ug_release_twin as tw

pytestmark = pytest.mark.gpu

FP32_TOL = dict(rtol=1e-4, atol=2e-5)       # the project's f32 tolerance of the sample pass (tests/test_gpu_parity.py)
HAND = orc.PlanarHandOracle
NE, STRIDE = 256, 116                       # csrc/smooth_ug.hip: the table
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ug_geometry_parent.npz")
SEED = 5


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return irs_mpc_amd


# ------------------------------------------------------------------------------------------------ the inputs
def projections(sys_o, x):
    """Per link-disc pair (arm 0 link 0, arm 0 link 1, arm 1 link 0, arm 1 link 1): the UNCLAMPED projection of the
    disc's centre on the link's axis and the link's length (the model clamps the projection to [0, L])."""
    q = x[HAND.PERM]
    out = []
    for arm in range(2):
        base = -sys_o.base_x if arm == 0 else sys_o.base_x
        a1 = q[3] + np.pi if arm == 0 else q[5]
        a2 = a1 + (q[4] if arm == 0 else q[6])
        p1 = np.array([np.cos(a1) * sys_o.l1 + base, np.sin(a1) * sys_o.l1])
        for link in range(2):
            a = np.array([base, 0.0]) if link == 0 else p1
            ang, L = (a1, sys_o.l1) if link == 0 else (a2, sys_o.l2)
            out.append((float((q[:2] - a).dot([np.cos(ang), np.sin(ang)])), L))
    return out


def clamp_states():
    """Two hand-made states: the disc behind the left arm's base (its first link's projection < 0) and the disc far
    above the hand (every projection beyond its link's end)."""
    behind = HAND.pack([0.3, 0.2, 0.1], [-np.pi / 4, -np.pi / 4], [np.pi / 4, np.pi / 4])
    beyond = HAND.pack([0.0, 0.9, -0.2], [-np.pi / 4, -np.pi / 4], [np.pi / 4, np.pi / 4])
    X = np.stack([behind, beyond])
    return X, X[:, tw.HAND_IDX] + np.array([[0.02, -0.01, 0.03, 0.01], [-0.02, 0.01, 0.0, 0.02]])


def states():
    """(X, U), 17 rows: states 0, 25, 49 of the benchmark's rollout, twelve of the random-state generator (separated,
    touching, deeply penetrating), the two clamp states."""
    _, x_trj, u_trj = tw.bench_rollout(orc)
    Xr, Ur = tw.random_states(HAND, np.random.default_rng(SEED), 12)
    Xc, Uc = clamp_states()
    return np.vstack([x_trj[[0, 25, 49]], Xr, Xc]), np.vstack([u_trj[[0, 25, 49]], Ur, Uc])


def dump_table(amd, x, u, first_order):
    from irs_mpc_amd import _lib
    dm = amd.PlanarHandDynamics(0.1).dm()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.irs_debug_ug_table.restype = ctypes.c_int
    lib.irs_debug_ug_table.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                       ctypes.c_void_p]
    par = np.ascontiguousarray(np.asarray(dm.params, np.float64))
    xx, uu = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(u, np.float64)
    out = np.zeros((NE, STRIDE), np.float32)
    rc = lib.irs_debug_ug_table(dm.model_id, par.ctypes.data, xx.ctypes.data, uu.ctypes.data, int(first_order),
                                out.ctypes.data)
    assert rc == 0, rc
    return out


def table_record(amd):
    """What the golden file holds, from the loaded library: entry0 (2 modes, states, 116) as uint32 and the SHA-256 of
    every table (2 modes, states, 32) as uint8."""
    X, U = states()
    entry0 = np.zeros((2, len(X), STRIDE), np.uint32)
    sha = np.zeros((2, len(X), 32), np.uint8)
    for mode in range(2):
        for k in range(len(X)):
            tab = dump_table(amd, X[k], U[k], bool(mode))
            entry0[mode, k] = tab[0].view(np.uint32)
            sha[mode, k] = np.frombuffer(hashlib.sha256(tab.tobytes()).digest(), np.uint8)
    return dict(X=X, U=U, entry0=entry0, sha256=sha)


# ------------------------------------------------------------------------------------------------ 1. same bits
def test_clamp_states_clamp():
    """The hand-made states do what they are for: a projection below 0 in the first, above the link's length in the
    second (no GPU needed, but it belongs to the golden's inputs)."""
    sys_o = HAND(0.1)
    X, _ = clamp_states()
    assert any(sp < 0.0 for sp, _ in projections(sys_o, X[0]))
    assert any(sp > L for sp, L in projections(sys_o, X[1]))
    Xs, _ = states()
    phi = np.stack([sys_o._qp(x[None], x[None, tw.HAND_IDX])[3][0] for x in Xs[3:15]])
    assert (phi.min(1) > 0.0).any() and (phi.min(1) < -0.1).any()        # separated and deeply penetrating ones


def test_table_bits_of_the_parent(amd):
    """Entry 0 of the table and the SHA-256 of the whole table, 17 states x 2 modes, against the bits the commit before
    the lane-parallel geometry produced (assemble on every lane)."""
    gold = np.load(GOLDEN)
    rec = table_record(amd)
    np.testing.assert_array_equal(rec["X"], gold["X"])                    # the golden's inputs are these inputs
    np.testing.assert_array_equal(rec["U"], gold["U"])
    diff = rec["entry0"] != gold["entry0"]
    for mode, k in zip(*np.nonzero(diff.any(2))):
        a = rec["entry0"][mode, k].view(np.float32).astype(np.float64)
        b = gold["entry0"][mode, k].view(np.float32).astype(np.float64)
        print("mode %d state %d: %d of %d elements differ, max |diff| %.3e" % (mode, k, diff[mode, k].sum(), STRIDE,
                                                                              np.abs(a - b).max()))
    sha_same = (rec["sha256"] == gold["sha256"]).all(2)
    print("entry 0: %d of %d bit-equal; whole table: %d of %d hashes equal" % (
        (~diff.any(2)).sum(), diff.shape[0] * diff.shape[1], sha_same.sum(), sha_same.size))
    assert not diff.any()
    assert sha_same.all()


# ------------------------------------------------------------------------------------------------ 2. small shapes
def _general(fn):
    """fn() with IRS_UG=0 (read per call): the general contact kernel."""
    os.environ["IRS_UG"] = "0"
    try:
        return fn()
    finally:
        os.environ.pop("IRS_UG", None)


def u_block_of_sums(so, n=7, m=4):
    """The ZERO_ORDER_B layout [Gram of du | du (f - xb)' | sum du] cut out of the oracle's z = [dx | du] layout."""
    d = n + m
    iu = np.triu_indices(d)
    ng = len(iu[0])
    gram = [q for q in range(ng) if iu[0][q] >= n]
    zdf = [ng + i * n + k for i in range(n, d) for k in range(n)]
    sz = [ng + d * n + i for i in range(n, d)]
    return so[:, gram + zdf + sz]


@pytest.fixture(scope="module")
def two_steps():
    _, x_trj, u_trj = tw.bench_rollout(orc)
    return x_trj[[0, 25]], u_trj[[0, 25]]


@pytest.mark.parametrize("source", ["supplied", "drawn"])
@pytest.mark.parametrize("N", [1, 64, 65, 600])
def test_small_shapes(amd, two_steps, N, source):
    """T = 2 (states 0 and 25 of the benchmark's rollout), std 0.5, both modes: the statistics against the oracle and the
    general kernel (zero-order: FP32_TOL; first-order, a sum of N piecewise-constant derivatives: 20 in the sum, the
    20 / N of tests/test_smooth_ug_table_gpu.py in the mean); from N = 64 on (the fit of B needs more than one sample)
    B and c likewise and info == 0; a second run bit-equal."""
    from irs_mpc_amd import device as dev
    from irs_mpc_amd._lib import SMOOTH_FIRST_ORDER, SMOOTH_ZERO_ORDER_B
    sys_o = HAND(0.1)
    X, U = two_steps
    xp = np.vstack([X, X[-1:]])
    dm = amd.PlanarHandDynamics(0.1).dm()
    xd, ud = dev.to_dev(X), dev.to_dev(U)
    su, seed, it = np.full(4, 0.5), 4321, 3
    if source == "supplied":
        du = (0.5 * np.random.default_rng(SEED + N).normal(size=(2, N, 4))).astype(np.float32)
        dud = dev.to_dev(du, dev.F32)

        def run(mode):
            return dm.smooth(mode, xd, ud, None, dud)
    else:
        du = dm.rng_samples(2, N, np.full(7, 0.05), su, seed, it)[1].cpu().numpy()

        def run(mode):
            return dm.smooth_rng(mode, xd, ud, N, None, su, seed, it)
    du64 = du.astype(np.float64)
    for mode in (SMOOTH_ZERO_ORDER_B, SMOOTH_FIRST_ORDER):
        keys = ("sums", "Bt", "ct", "info")
        got = {k: v.cpu().numpy() for k, v in run(mode).items() if k in keys}
        gen = {k: v.cpu().numpy() for k, v in _general(lambda: run(mode)).items() if k in keys}
        again = {k: v.cpu().numpy() for k, v in run(mode).items() if k in keys}
        for k in keys:
            assert np.array_equal(got[k], again[k], equal_nan=True), k
        if mode == SMOOTH_ZERO_ORDER_B:
            so = u_block_of_sums(orc.zero_order_sums(sys_o, X, U, np.zeros((2, N, 7)), du64, sum_z=True))
            print("N %d %s zero-order-B: |sums - oracle| %.2e |sums - general| %.2e" % (
                N, source, np.abs(got["sums"] - so).max(), np.abs(got["sums"] - gen["sums"]).max()))
            np.testing.assert_allclose(got["sums"], so, **FP32_TOL)
            np.testing.assert_allclose(got["sums"], gen["sums"], **FP32_TOL)
        else:
            so = orc.first_order_sums(sys_o, X, U, du64)
            print("N %d %s first-order: |sums - oracle| %.2e |sums - general| %.2e (bound 20)" % (
                N, source, np.abs(got["sums"] - so).max(), np.abs(got["sums"] - gen["sums"]).max()))
            assert np.abs(got["sums"] - so).max() < 20.0
            assert np.abs(got["sums"] - gen["sums"]).max() < 20.0
        if N < 64:
            continue
        assert int(np.abs(got["info"]).sum()) == 0
        if mode == SMOOTH_ZERO_ORDER_B:
            _, Bo, co = orc.zero_order_B_decoupled(sys_o, xp, U, du64)
            print("N %d %s zero-order-B: |B - oracle| %.2e |c - oracle| %.2e |B - general| %.2e" % (
                N, source, np.abs(got["Bt"] - Bo).max(), np.abs(got["ct"] - co).max(), np.abs(got["Bt"] - gen["Bt"]).max()))
            for ref in ((Bo, co), (gen["Bt"], gen["ct"])):
                np.testing.assert_allclose(got["Bt"], ref[0], **FP32_TOL)
                np.testing.assert_allclose(got["ct"], ref[1], **FP32_TOL)
        else:
            _, Bo, _ = orc.first_order_B_decoupled(sys_o, xp, U, du64)
            print("N %d %s first-order: |B - oracle| %.2e |B - general| %.2e (bound %.2e)" % (
                N, source, np.abs(got["Bt"] - Bo).max(), np.abs(got["Bt"] - gen["Bt"]).max(), 20.0 / N))
            assert np.abs(got["Bt"] - Bo).max() < 20.0 / N
            assert np.abs(got["Bt"] - gen["Bt"]).max() < 20.0 / N


def test_solo_versus_batch(amd, two_steps):
    """Two problems on the same rows in one launch (B = 2, N = 65, drawn samples), each bit-equal to its solo launch, in
    both modes."""
    from irs_mpc_amd import device as dev
    from irs_mpc_amd._lib import SMOOTH_FIRST_ORDER, SMOOTH_ZERO_ORDER_B
    X, U = two_steps
    dm = amd.PlanarHandDynamics(0.1).dm()
    xd, ud = dev.to_dev(X), dev.to_dev(U)
    Xb, Ub = dev.to_dev(np.stack([X, X])), dev.to_dev(np.stack([U, U]))
    std, seeds, N = np.array([[0.5] * 4, [0.2] * 4]), [1234, 99], 65
    for mode in (SMOOTH_ZERO_ORDER_B, SMOOTH_FIRST_ORDER):
        ob = dm.smooth_rng_batch(mode, Xb, Ub, N, dev.to_dev(std), torch.tensor(seeds, dtype=torch.int64, device="cuda"), 1)
        assert int(ob["info"].abs().sum().item()) == 0
        for b in range(2):
            os_ = dm.smooth_rng(mode, xd, ud, N, None, std[b], seeds[b], 1)
            for kk in ("At", "Bt", "ct"):
                assert torch.equal(ob[kk][b], os_[kk]), (b, kk)
