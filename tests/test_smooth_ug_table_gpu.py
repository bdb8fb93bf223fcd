"""The active-set table of the uniform-geometry sample pass, built by pivot steps (csrc/smooth_ug.hip, ug_build_table).

Entry A of the table is G_A [r0 | C' | W] (zero-order pass) or [G_A r0 | G_A C' | G_A] (first-order pass), with G_A the
map r -> [lam on the reduced set ; slacks off it]; the kernel reaches it from the empty set by one rank-1 pivot per row
of A, in row order, a row whose pivot is below 1e-5 W_pp dropping out.  Three views:

1. every entry of six states' tables (irs_debug_ug_table) against the f64 definition;
2. a state with an exactly repeated contact row: the later row drops out of every set that has both;
3. the sample pass end to end at the smallest shapes with trips, a flush and two workgroups, solo and batched.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import irs_oracle as orc

pytestmark = pytest.mark.gpu

FP32_TOL = dict(rtol=1e-4, atol=2e-5)       # the project's f32 tolerance of the sample pass (tests/test_gpu_parity.py)
HAND = orc.PlanarHandOracle
HAND_IDX = np.array([1, 4, 2, 5])
PIVOT = 1e-5                                # csrc/smooth_ug.hip: the table's pivot rule
NE, STRIDE, TAB_H, TAB_TAU, TAB_SET, TAB_X = 256, 116, 8, 40, 48, 52      # csrc/smooth_ug.hip: kUgTab*
SEED = 7
# Value error e = max|got - exact| / max|exact| of an entry, over the compared (non-borderline) entries of the six states
# in both modes, measured on an MI355X through irs_debug_ug_table:
#   one masked LDL' per entry (-DIRS_UG_TABLE_LDL=1):  max e 2.361e-3, mean e 1.617e-5
#   pivot steps (the product build):                    max e 2.619e-3, mean e 1.649e-5
# The pivot build may exceed neither by more than the factor 2 (rounding-order noise).
LDL_MAX_E = 2.361e-3
LDL_MEAN_E = 1.617e-5


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return irs_mpc_amd


# ------------------------------------------------------------------------------------------------ the inputs
def bench_rollout():
    sys_o = HAND(0.1)
    x0 = HAND.pack([0.0, 0.35, 0.0], [-np.pi / 4, -np.pi / 4], [np.pi / 4, np.pi / 4])
    u_trj = np.tile(x0[HAND_IDX], (50, 1))
    return orc.rollout(sys_o, x0, u_trj), u_trj


def random_rows(rng, k):
    """The generator of tests/test_smooth_ug_affine_gpu.py: separated, touching, deeply penetrating."""
    obj = np.stack([rng.uniform(-0.3, 0.3, k), rng.uniform(0.1, 0.7, k), rng.uniform(-1, 1, k)], 1)
    left = np.stack([rng.uniform(-2.2, -0.2, k), rng.uniform(-1.5, 0.5, k)], 1)
    right = np.stack([rng.uniform(0.2, 2.2, k), rng.uniform(-0.5, 1.5, k)], 1)
    X = np.zeros((k, 7))
    X[:, HAND.PERM] = np.hstack([obj, left, right])
    U = X[:, HAND_IDX] + rng.normal(0, 0.1, (k, 4))
    return X, U


def dual_problem(sys_o, x, u):
    """W (8,8), r0 (8,), C (8,4: r = r0 + C du) and phi (8,) of the step QP's dual at one state and command, in f64."""
    def wr(uu):
        Dinv, b, J, phi = sys_o._qp(x[None], uu[None])
        JD = J[0] * Dinv
        return JD.dot(J[0].T), phi[0] - JD.dot(b[0]), phi[0]
    W, r0, phi = wr(u)
    C = np.stack([wr(u + np.eye(4)[j])[1] - r0 for j in range(4)], 1)       # r is affine in the command
    return W, r0, C, phi


def table_states():
    """States 0 and 25 of the benchmark's rollout and the first four of the generator (seed 7) whose tables have at most
    8 borderline entries, a deeply penetrating one (phi < -0.1 on some row) among them."""
    sys_o = HAND(0.1)
    x_trj, u_trj = bench_rollout()
    states = [(x_trj[0], u_trj[0]), (x_trj[25], u_trj[25])]
    X, U = random_rows(np.random.default_rng(SEED), 80)
    picked, deep = [], False
    for k in range(80):
        W, r0, C, phi = dual_problem(sys_o, X[k], U[k])
        nb = sum(definition(W, r0, C, a, False)[3] for a in range(NE))
        is_deep = phi.min() < -0.1
        if nb > 8 or (len(picked) == 3 and not deep and not is_deep):
            continue
        picked.append((X[k], U[k]))
        deep = deep or is_deep
        if len(picked) == 4:
            break
    assert len(picked) == 4 and deep
    return states + picked


# ------------------------------------------------------------------------------------------------ the definition
def definition(W, r0, C, a, first_order):
    """Entry `a` in f64: (reduced set as a bool mask, h | H (8 x 5), X (8 x 8), borderline).  Row-order elimination: row
    j of `a` enters the set if its Schur complement d on the rows accepted so far exceeds PIVOT W_jj; borderline if
    some d / W_jj lies in (1e-6, 1e-4)."""
    nc = len(r0)
    S, borderline = [], False
    for j in range(nc):
        if not (a >> j) & 1:
            continue
        d = W[j, j] - (W[j, S].dot(np.linalg.solve(W[np.ix_(S, S)], W[S, j])) if S else 0.0)
        borderline = borderline or 1e-6 < d / W[j, j] < 1e-4
        if d > PIVOT * W[j, j]:
            S.append(j)
    on = np.zeros(nc, bool)
    on[S] = True
    G = np.eye(nc)
    if S:
        Minv = -np.linalg.inv(W[np.ix_(S, S)])
        G[:, S] = 0.0
        G[np.ix_(S, S)] = Minv
        off = np.where(~on)[0]
        G[np.ix_(off, S)] = W[np.ix_(off, S)].dot(Minv)
        G[S] *= on                                              # rows of the set: nothing off it
    hH = G.dot(np.column_stack([r0, C]))
    if first_order:
        return on, hH, G, borderline
    X = G.dot(W)
    for p in S:                                                 # columns of the set: -e_p, exactly
        X[:, p] = 0.0
        X[p, p] = -1.0
    return on, hH, X, borderline


def u_block_of_sums(so, n=7, m=4):
    """The ZERO_ORDER_B layout [Gram of du | du (f - xb)' | sum du] cut out of the oracle's z = [dx | du] layout."""
    d = n + m
    iu = np.triu_indices(d)
    ng = len(iu[0])
    gram = [q for q in range(ng) if iu[0][q] >= n]
    zdf = [ng + i * n + k for i in range(n, d) for k in range(n)]
    sz = [ng + d * n + i for i in range(n, d)]
    return so[:, gram + zdf + sz]


def dump_table(amd, x, u, first_order, dm=None):
    from irs_mpc_amd import _lib
    dm = dm or amd.PlanarHandDynamics(0.1).dm()
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


def table_errors(amd, states=None):
    """Per mode and state: checks sets and tau of every entry, returns the value errors e of the compared entries and
    the number of borderline ones."""
    sys_o = HAND(0.1)
    errs, borderline, total = [], [], 0
    for first_order in (False, True):
        for x, u in (states or table_states()):
            W, r0, C, _ = dual_problem(sys_o, x, u)
            tab = dump_table(amd, x, u, first_order)
            nb = 0
            for a in range(NE):
                e = tab[a]
                got_set = int(e[TAB_SET:TAB_SET + 1].view(np.uint32)[0])
                tau = e[TAB_TAU:TAB_TAU + 8]
                on, hH, X, bl = definition(W, r0, C, a, first_order)
                # internal consistency, every entry: a subset of `a`, tau = 0 exactly on it
                assert got_set & ~a == 0
                assert np.array_equal(tau, np.array([0.0 if (got_set >> i) & 1 else 1.0 for i in range(8)], np.float32))
                total += 1
                if bl:
                    nb += 1
                    continue
                assert got_set == sum(1 << i for i in range(8) if on[i]), (a, got_set, on)
                got = np.column_stack([e[:TAB_TAU].reshape(5, 8).T, e[TAB_X:].reshape(8, 8).T]).astype(np.float64)
                exact = np.column_stack([hH, X])
                errs.append(np.abs(got - exact).max() / np.abs(exact).max())
            borderline.append(nb)
    return np.array(errs), borderline, total


# ------------------------------------------------------------------------------------------------ the tests
def test_every_entry_against_its_definition(amd):
    """All 256 entries of six states, both modes, against the f64 definition on the f64 geometry: the reduced set and tau
    exactly, the values (the never-read columns p in A of the zero-order X included, against -e_p) within twice the error
    of the one-LDL'-per-entry build on the same inputs.  Borderline entries (a candidate pivot within a decade of the
    rule) are held to the consistency of tau and the set only: at most 8 per table, 1 % overall.
    Measured on an MI355X over the 3 060 compared entries (12 of 3 072 borderline, at most 4 in a table): the LDL' build
    max e 2.361e-3, mean e 1.617e-5 (LDL_MAX_E, LDL_MEAN_E); the pivot build max e 2.619e-3, mean e 1.649e-5 -- ratios
    1.11 and 1.02 against the bound 2."""
    errs, borderline, total = table_errors(amd)
    print("table: %d entries, %d borderline (worst table %d); e max %.3e mean %.3e" % (
        total, sum(borderline), max(borderline), errs.max(), errs.mean()))
    assert max(borderline) <= 8 and sum(borderline) <= 0.01 * total
    assert errs.max() <= 2 * LDL_MAX_E
    assert errs.mean() <= 2 * LDL_MEAN_E


MU_DEP = 0.0


def dependent_state():
    """Without friction the two generators n +- mu t of a contact coincide: rows 2k and 2k + 1 of J, and so of W, are
    equal to the bit at every state.  State 25 of the benchmark's rollout (the disc rests on the links) under mu = 0."""
    sys_o = HAND(0.1, mu=MU_DEP)
    x_trj, u_trj = bench_rollout()
    x, u = x_trj[25], u_trj[25]
    W = dual_problem(sys_o, x, u)[0]
    same = [(i, j) for i in range(8) for j in range(i + 1, 8) if np.array_equal(W[i], W[j])]
    assert same == [(0, 1), (2, 3), (4, 5), (6, 7)]
    return sys_o, x, u, same


def test_dependent_rows_drop_out(amd):
    """A state whose W repeats contact rows exactly (no friction: both generators of a contact are its normal): every
    candidate set with both rows of a pair, the full set included, keeps the earlier and drops the later one, in both
    modes; and through dm.smooth_accumulate at N = 1, samples whose optimal set loads such rows meet the oracle to
    FP32_TOL."""
    from irs_mpc_amd import device as dev
    from irs_mpc_amd._lib import SMOOTH_ZERO_ORDER_B
    sys_o, x, u, same = dependent_state()
    dm = amd.PlanarHandDynamics(0.1, mu=MU_DEP).dm()
    for first_order in (False, True):
        tab = dump_table(amd, x, u, first_order, dm)
        sets = tab[:, TAB_SET].copy().view(np.uint32)
        assert int(sets[255]) == 0b01010101
        for i, j in same:
            for a in range(NE):
                if (a >> i) & 1 and (a >> j) & 1:
                    assert (int(sets[a]) >> i) & 1 and not (int(sets[a]) >> j) & 1, (a, sets[a])
                    assert tab[a, TAB_TAU + i] == 0.0 and tab[a, TAB_TAU + j] == 1.0
    K = 64
    du = (0.5 * np.random.default_rng(SEED).normal(size=(K, 1, 4))).astype(np.float32)
    X, U = np.tile(x, (K, 1)), np.tile(u, (K, 1))
    loaded = 0
    for k in range(K):
        Dinv, b, J, phi = sys_o._qp(x[None], (u + du[k, 0].astype(np.float64))[None])
        JD = J[0] * Dinv
        lam = sys_o._dual_exact(JD.dot(J[0].T)[None], (phi[0] - JD.dot(b[0]))[None])[0]
        loaded += bool((lam > 0).any())
    print("%d of %d samples load a repeated row" % (loaded, K))
    assert loaded >= 8
    so = u_block_of_sums(orc.zero_order_sums(sys_o, X, U, np.zeros((K, 1, 7)), du.astype(np.float64), sum_z=True))
    got = dm.smooth_accumulate(SMOOTH_ZERO_ORDER_B, dev.to_dev(X), dev.to_dev(U), None, dev.to_dev(du, dev.F32)).cpu().numpy()
    err = np.abs(got - so)
    print("max |sums - oracle| %.3e, in units of the tolerance %.3f" % (
        err.max(), (err / (FP32_TOL["atol"] + FP32_TOL["rtol"] * np.abs(so))).max()))
    np.testing.assert_allclose(got, so, **FP32_TOL)


@pytest.mark.parametrize("N", [200, 700], ids=["one_workgroup", "two_workgroups"])
def test_sample_pass_end_to_end(amd, N):
    """T = 3 (states 0, 25, 49 of the benchmark's rollout), N = 200 (trips and the flush in one workgroup) and N = 700 (two
    workgroups per time step), std 0.5, both modes: against the oracle to the tolerances of
    test_trips_and_flush_vs_oracle_and_general_kernel, info == 0, a second run bit-equal; and the batch entry point at
    B = 2 on the same rows, both problems bit-equal to the solo launch with their seed."""
    from irs_mpc_amd import device as dev
    from irs_mpc_amd._lib import SMOOTH_FIRST_ORDER, SMOOTH_ZERO_ORDER_B
    sys_o = HAND(0.1)
    x_trj, u_trj = bench_rollout()
    X, U = x_trj[[0, 25, 49]], u_trj[[0, 25, 49]]
    xp = np.vstack([X, X[-1:]])
    du = (0.5 * np.random.default_rng(11).normal(size=(3, N, 4))).astype(np.float32)
    dm = amd.PlanarHandDynamics(0.1).dm()
    xd, ud, dud = dev.to_dev(X), dev.to_dev(U), dev.to_dev(du, dev.F32)
    for mode in (SMOOTH_ZERO_ORDER_B, SMOOTH_FIRST_ORDER):
        o = dm.smooth(mode, xd, ud, None, dud)
        Bt, ct, info = o["Bt"].cpu().numpy(), o["ct"].cpu().numpy(), o["info"].cpu().numpy()
        assert int(np.abs(info).sum()) == 0
        if mode == SMOOTH_ZERO_ORDER_B:
            _, Bo, co = orc.zero_order_B_decoupled(sys_o, xp, U, du.astype(np.float64))
            print("N %d zero-order-B: |B - oracle| %.2e |c - oracle| %.2e" % (N, np.abs(Bt - Bo).max(), np.abs(ct - co).max()))
            np.testing.assert_allclose(Bt, Bo, **FP32_TOL)
            np.testing.assert_allclose(ct, co, **FP32_TOL)
        else:
            _, Bo, _ = orc.first_order_B_decoupled(sys_o, xp, U, du.astype(np.float64))
            print("N %d first-order: |B - oracle| %.2e (bound %.2e)" % (N, np.abs(Bt - Bo).max(), 20.0 / N))
            assert np.abs(Bt - Bo).max() < 20.0 / N
        o2 = dm.smooth(mode, xd, ud, None, dud)
        assert np.array_equal(o2["Bt"].cpu().numpy(), Bt) and np.array_equal(o2["ct"].cpu().numpy(), ct)
        # two problems on the same rows in one launch, each against its solo launch
        std = np.full((2, 4), 0.5)
        seeds = [1234, 99]
        Xb, Ub = dev.to_dev(np.stack([X, X])), dev.to_dev(np.stack([U, U]))
        ob = dm.smooth_rng_batch(mode, Xb, Ub, N, dev.to_dev(std), torch.tensor(seeds, dtype=torch.int64, device="cuda"), 1)
        assert int(ob["info"].abs().sum().item()) == 0
        for b in range(2):
            os_ = dm.smooth_rng(mode, xd, ud, N, None, std[b], seeds[b], 1)
            for kk in ("At", "Bt", "ct"):
                assert torch.equal(ob[kk][b], os_[kk]), (b, kk)
