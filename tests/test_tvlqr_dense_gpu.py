"""Dense and unsymmetric cost weights through every kernel that reads Q, Qd or R.

Every other GPU test hands the library diagonal weights, under which a transposed read, a kernel that picks up
only the diagonal, or a wrong off-diagonal term in -Q xd_t gives the right answer.  Here the weights are dense
(three families: SPD, PSD with a null space that is not axis-aligned, badly scaled), the Riccati pass is run on
each of its four implementations (registers, matrix cores, the LDS recursion the matrix-core sizes fall back to
beyond (T + 1) n = 4096, and the runtime-size kernel) against the extended-precision reference of
oracle/tvlqr_highprec.py, and the same weights go through the rollout / cost kernels, the ADMM, both active-set
descents, the CEM cost kernels and the fused iterate.

Unsymmetric weights (`skew`: W + a (S - S'); `triu`: the upper-triangle spelling) must give the result of their
symmetric part (include/irs_hip.h), at rtol 1e-12.  The inputs sit on a 2^-30 grid, on which the symmetric part of
either spelling is the symmetric weight bit for bit (tvlqr_highprec.on_grid), so the comparison sees the kernel's
treatment of the skew part and not an amplified rounding of (s + k) + (s - k).

Tolerances are the suite's own for f64 device results: rtol 1e-8 / atol 1e-9 on gains, plans and trajectories,
rtol 1e-12 on costs.  tests/test_tvlqr_reference_cpu.py admits each input only if the f64 oracle is within 1/100
of that of the extended-precision answer.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import irs_oracle as orc
from oracle import tvlqr_highprec as hp

pytestmark = pytest.mark.gpu

TOL = hp.GPU_TOL
SAME = dict(rtol=1e-12, atol=0)              # unsymmetric spelling vs its symmetric part
VARIANTS = ("sym", "skew", "triu")


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()     # fails loudly if the HIP library is missing
    return irs_mpc_amd


@pytest.fixture(params=[2, 3], ids=["lanes", "mfma"])
def as_solver(request):
    """The two device implementations of the exact active-set descent (include/irs_hip.h, `solver`):
    2 = ctrlbox.hip (lanes + LDS), 3 = ctrlbox_mfma.hip (matrix-core tiles)."""
    return request.param


def spelled(p, variant):
    """(Q, Qd, R) of a problem dict in one of the three spellings."""
    return (p["Q"], p["Qd"], p["R"]) if variant == "sym" else p["unsym"][variant]


def unsym_of(Q, Qd, R, seed):
    rng = np.random.default_rng(seed)
    v = [hp.skew_variants(W, rng) for W in (Q, Qd, R)]
    return {name: tuple(w[name] for w in v) for name in ("skew", "triu")}


def npy(t):
    return t.cpu().numpy()


def report(what, got, want, **tol):
    """Print the figure, then assert it."""
    tol = tol or TOL
    got, want = np.asarray(got, float), np.asarray(want, float)
    err = np.abs(got - want)
    print("%s: max abs err %.3g, worst err / (atol + rtol |want|) %.3g" % (
        what, err.max(), (err / np.maximum(tol.get("atol", 0) + tol["rtol"] * np.abs(want), 1e-300)).max()))
    np.testing.assert_allclose(got, want, err_msg=what, **tol)


# ---------------------------------------------------------------- B1 / B3: irs_tvlqr_riccati on every path
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("family", hp.FAMILIES)
@pytest.mark.parametrize("n,m,T,impl", hp.RICCATI_CASES, ids=["%s-n%d-m%d-T%d" % (c[3], c[0], c[1], c[2])
                                                              for c in hp.RICCATI_CASES])
def test_riccati_dense_weights_vs_extended_precision(amd, n, m, T, impl, family, variant):
    from irs_mpc_amd import device as dev
    p = hp.riccati_problem(n, m, T, family)
    K, k = hp.riccati_reference(n, m, T, family)
    lin = [dev.to_dev(p[a]) for a in ("At", "Bt", "ct")]
    xd = dev.to_dev(p["xd"])

    def run(v):
        Kd, kd, info = dev.tvlqr_riccati(*lin, *[dev.to_dev(W) for W in spelled(p, v)], xd, alpha_R=0.5)
        assert int(info.item()) == 0, (v, int(info.item()))
        return npy(Kd), npy(kd)

    Kd, kd = run(variant)
    report("K vs extended precision", Kd, K.astype(float))
    report("k vs extended precision", kd, k.astype(float))
    if variant != "sym":
        Ks, ks = run("sym")
        report("K, %s vs symmetric part" % variant, Kd, Ks, **SAME)
        report("k, %s vs symmetric part" % variant, kd, ks, **SAME)


@pytest.mark.parametrize("n,m,T,impl", [(2, 1, 30, "registers"), (5, 2, 40, "mfma"), (5, 2, 819, "lds"),
                                        (3, 2, 17, "generic")], ids=lambda v: str(v))
def test_riccati_reports_an_indefinite_cost_on_every_path(amd, n, m, T, impl):
    """A concave state cost under a vanishing control weight: H = alpha R + B'PB is not positive definite at the
    first step already, and each of the four implementations says so through info."""
    from irs_mpc_amd import device as dev
    p = hp.riccati_problem(n, m, T, "spd")
    args = [dev.to_dev(a) for a in (p["At"], p["Bt"], p["ct"], -50.0 * p["Q"], -50.0 * p["Qd"], 1e-6 * p["R"], p["xd"])]
    _, _, info = dev.tvlqr_riccati(*args, alpha_R=0.5)
    assert int(info.item()) != 0
    H = 0.5e-6 * p["R"] - 50.0 * p["Bt"][T - 1].T.dot(p["Qd"]).dot(p["Bt"][T - 1])
    assert np.linalg.eigvalsh(H).min() < 0


# ---------------------------------------------------------------- B2 / B3: rollouts, costs, the fused descent
def _device_system(amd, name, h):
    return {"pendulum": amd.PendulumDynamics, "bicycle": amd.BicycleDynamics, "three_cart": amd.ThreeCartDynamics,
            "quadrotor": amd.QuadrotorDynamics}[name](h)


def _model_run(amd, name, h, T, variant):
    """evaluate_cost, rollout_cost, tvlqr_descent and closed_loop_rollout of one model problem in one spelling."""
    from irs_mpc_amd import device as dev
    p = hp.model_problem(name, h, T)
    dm = _device_system(amd, name, h).dm()
    n, m = p["At"].shape[1], p["Bt"].shape[2]
    Q, Qd, R = (dev.to_dev(W) for W in spelled(p, variant))
    xd, x0 = dev.to_dev(p["xd"]), dev.to_dev(p["x0"])
    rng = np.random.default_rng(T)
    xr, ur = rng.normal(size=(T + 1, n)), rng.normal(size=(T, m))
    out = dict(xr=xr, ur=ur)
    out["cost_eval"] = float(dev.evaluate_cost(dev.to_dev(xr), dev.to_dev(ur), Q, R, xd).item())
    xt, c = dm.rollout_cost(x0, dev.to_dev(p["u_trj"]), Q, R, xd)
    out["x_roll"], out["cost_roll"] = npy(xt), float(c.item())
    o = dm.tvlqr_descent(*[dev.to_dev(p[a]) for a in ("At", "Bt", "ct")], Q, Qd, R, xd, x0)
    assert int(o["info"].item()) == 0
    out.update(K=npy(o["K"]), k=npy(o["k"]), x_new=npy(o["x_new"]), u_new=npy(o["u_new"]), cost=float(o["cost"].item()))
    Ko, ko = orc.tvlqr_riccati(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["xd"])
    x2, u2, c2 = dm.closed_loop_rollout(dev.to_dev(Ko), dev.to_dev(ko), x0, Q, R, xd)
    out.update(Ko=Ko, ko=ko, x_cl=npy(x2), u_cl=npy(u2), cost_cl=float(c2.item()))
    return out


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name,h,T", hp.MODEL_CASES, ids=["%s-T%d%s" % (c[0], c[2], "-lds-fallback" if c[2] > 340 else "")
                                                          for c in hp.MODEL_CASES])
def test_cost_rollout_and_descent_dense_weights(amd, name, h, T, variant):
    """irs_evaluate_cost, irs_rollout_cost, irs_closed_loop_rollout and the fused irs_tvlqr_descent (pendulum: the
    register Riccati and rollout; quadrotor T = 341: the LDS fallback inside the descent kernel) with dense weights:
    gains against the extended-precision reference, trajectories against the oracle's descent, costs against
    the oracle's evaluate_cost of the same trajectories."""
    p = hp.model_problem(name, h, T)
    s = p["sys_o"]
    g = _model_run(amd, name, h, T, variant)
    Qs, Rs = p["Q"], p["R"]
    report("evaluate_cost", g["cost_eval"], orc.evaluate_cost(g["xr"], g["ur"], p["xd"], Qs, Rs), rtol=1e-12)
    report("rollout_cost x_trj", g["x_roll"], p["x_trj"])
    report("rollout_cost cost", g["cost_roll"], orc.evaluate_cost(g["x_roll"], p["u_trj"], p["xd"], Qs, Rs), rtol=1e-12)
    K, k = hp.tvlqr_riccati(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["xd"])
    report("descent K vs extended precision", g["K"], K.astype(float))
    report("descent k vs extended precision", g["k"], k.astype(float))
    xo, uo, _, _ = orc.local_descent(s, p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["x0"], p["xd"])
    report("descent u_new", g["u_new"], uo)
    report("descent x_new", g["x_new"], xo)
    report("descent cost", g["cost"], orc.evaluate_cost(g["x_new"], g["u_new"], p["xd"], Qs, Rs), rtol=1e-12)
    x2, u2 = orc.closed_loop_rollout(s, g["Ko"], g["ko"], p["x0"])
    report("closed_loop_rollout u", g["u_cl"], u2)
    report("closed_loop_rollout x", g["x_cl"], x2)
    report("closed_loop_rollout cost", g["cost_cl"], orc.evaluate_cost(g["x_cl"], g["u_cl"], p["xd"], Qs, Rs), rtol=1e-12)
    if variant != "sym":
        b = _model_run(amd, name, h, T, "sym")
        for key in ("cost_eval", "x_roll", "cost_roll", "K", "k", "x_new", "u_new", "cost", "x_cl", "u_cl", "cost_cl"):
            report("%s, %s vs symmetric part" % (key, variant), g[key], b[key], **SAME)


# ---------------------------------------------------------------- B2 / B3: ADMM (csrc/boxqp.hip)
@functools.lru_cache(maxsize=None)
def _admm_plain_problem():
    """The bicycle's model problem with a steer bound and an input bound at half of what the unconstrained plan
    (extended-precision reference) reaches: both bind."""
    p = hp.model_problem("bicycle", 0.1, 25)
    T = 25
    xs, us = hp.solve_tvlqr(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["x0"], p["xd"])
    steer, ubnd = 0.5 * float(np.abs(xs[1:, 4]).max()), 0.5 * float(np.abs(us[:, 0]).max())
    xhi, uhi = np.array([1e4, 1e4, 1e4, 1e4, steer]), np.array([ubnd, 1e4])
    F = orc.tvlqr_box_factor(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], -xhi, xhi, -uhi, uhi, 10.0, alpha_R=0.5)
    zx, zu, _, it = orc.tvlqr_box_solve(F, p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["xd"], p["x0"], 0, -xhi, xhi,
                                        -uhi, uhi, None, 40000, 1e-10, 1.6)
    return dict(p=p, T=T, xhi=xhi, uhi=uhi, zx=zx, zu=zu, it=it, xs=xs.astype(float), us=us.astype(float))


@pytest.mark.parametrize("variant", VARIANTS)
def test_admm_plain_form_dense_weights(amd, variant):
    """One bounded QP in the plain form (bicycle, alpha_R = 1/2), dense weights, state and input bound active:
    certified by the QP's KKT conditions (independent of any solver) and equal to the oracle's ADMM solution."""
    a = _admm_plain_problem()
    p, T, xhi, uhi = a["p"], a["T"], a["xhi"], a["uhi"]
    assert a["it"] < 40000
    xb = np.stack([np.tile(-xhi, (T + 1, 1)), np.tile(xhi, (T + 1, 1))])
    ub = np.stack([np.tile(-uhi, (T, 1)), np.tile(uhi, (T, 1))])

    def run(v):
        Q, Qd, R = spelled(p, v)
        return amd.solve_tvlqr(p["At"], p["Bt"], p["ct"], Q, Qd, R, p["x0"], p["xd"], amd.get_solver("osqp"),
                               x_bound_abs=xb, u_bound_abs=ub, eps=1e-10, max_iter=40000)

    xs, us = run(variant)
    assert np.abs(us[:, 0]).max() > uhi[0] - 1e-6 and np.abs(xs[1:, 4]).max() > xhi[4] - 1e-6      # both bind
    assert np.abs(us - a["us"]).max() > 1e-2                                                       # and it matters
    res = orc.qp_box_kkt_residuals(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["x0"], p["xd"], -xhi, xhi,
                                   -uhi, uhi, xs, us, alpha_R=0.5)
    print("KKT residuals (dynamics, box, stationarity, multiplier sign):", res)
    assert max(res) < 1e-5, res
    report("u* vs oracle ADMM", us, a["zu"], rtol=0, atol=1e-7)
    report("x* vs oracle ADMM", xs, a["zx"], rtol=0, atol=1e-7)
    if variant != "sym":
        x0s, u0s = run("sym")
        report("u*, %s vs symmetric part" % variant, us, u0s, **SAME)
        report("x*, %s vs symmetric part" % variant, xs, x0s, **SAME)


HAND = orc.PlanarHandOracle
HAND_IDX = np.array([1, 4, 2, 5])        # indices_u_into_x in the reference's state order
HAND_Q = HAND.pack([1e-3, 1e-3, 10.0], [1e-3, 1e-3], [1e-3, 1e-3])          # run_planar_hand.py:113-121
HAND_GOAL = HAND.pack([0.3, -0.1, 0.5], [0, 0], [0, 0])                     # :123-125


def _hand_start():
    sys_o = orc.PlanarHandOracle(0.1)
    x0 = HAND.pack([0.0, 0.35, 0.0], [-np.pi / 4, -np.pi / 4], [np.pi / 4, np.pi / 4])   # run_planar_hand.py:31-44
    for _ in range(4):
        x0 = sys_o.dynamics(x0, np.array([-np.pi / 4, -np.pi / 4, np.pi / 4, np.pi / 4]))
    return sys_o, x0


def _hand_weights(rng, q, qd_scale, r):
    """V diag(q) V' with V a random rotation of all seven coordinates (object and fingers mixed), Qd likewise, and
    a dense SPD R with eigenvalues r; on the grid."""
    V = hp._rotation(rng, 7)
    Q = hp.on_grid((V * q).dot(V.T))
    Q = hp.on_grid(0.5 * (Q + Q.T))
    Vr = hp._rotation(rng, 4)
    R = hp.on_grid((Vr * r).dot(Vr.T))
    return Q, hp.on_grid(qd_scale * Q), hp.on_grid(0.5 * (R + R.T))


@functools.lru_cache(maxsize=None)
def _admm_du_problem():
    """The first tail QP of the planar hand's descent (position-controlled form: cost on du, trust region + rate
    limit), dense weights, and the oracle's ADMM solution of it on the [x; u_prev] augmentation."""
    T = 10
    sys_o, x0 = _hand_start()
    idx = sys_o.indices_u_into_x
    u_trj = np.tile(x0[HAND_IDX], (T, 1))
    x_trj = orc.rollout(sys_o, x0, u_trj)
    du = (np.random.default_rng(77).normal(size=(T, 300, 4)) * 0.1).astype(np.float32)
    A, B, c = orc.zero_order_B_decoupled(sys_o, x_trj, u_trj, du.astype(np.float64))
    rng = np.random.default_rng(78)
    Q, Qd, R = _hand_weights(rng, HAND_Q, 100.0, np.array([2.0, 4.0, 6.0, 9.0]))
    xd = np.tile(x0 + HAND_GOAL, (T + 1, 1))
    rows = orc.quasistatic_bounds(x_trj, idx, None, np.array([-np.ones(4) * 0.05, np.ones(4) * 0.05]),
                                  np.array([-np.ones(4) * 0.03, np.ones(4) * 0.03]))
    Ab, Bb, cb, Qb, Qdb, xdb = orc.quasistatic_augment(A, B, c, Q, Qd, xd)
    zlo = np.hstack([rows[0], np.vstack([np.full((1, 4), -np.inf), rows[2]])])
    zhi = np.hstack([rows[1], np.vstack([np.full((1, 4), np.inf), rows[3]])])
    F = orc.tvlqr_box_factor(Ab, Bb, cb, Qb, Qdb, R, zlo, zhi, rows[4], rows[5], 100.0, alpha_R=1.0)
    z0 = np.concatenate([x0, x0[idx]])
    zx, zu, _, it = orc.tvlqr_box_solve(F, Ab, Bb, cb, Qb, Qdb, xdb, z0, 0, zlo, zhi, rows[4], rows[5], None, 40000,
                                        1e-10, 1.6)
    res = orc.qp_box_kkt_residuals(Ab, Bb, cb, Qb, Qdb, R, z0, xdb, zlo, zhi, rows[4], rows[5], zx, zu, alpha_R=1.0)
    return dict(T=T, idx=idx, x0=x0, A=A, B=B, c=c, Q=Q, Qd=Qd, R=R, xd=xd, rows=rows, zx=zx, zu=zu, it=it, res=res,
                aug=(Ab, Bb, cb, Qb, Qdb, xdb, z0, zlo, zhi), unsym=unsym_of(Q, Qd, R, 79))


@pytest.mark.parametrize("variant", VARIANTS)
def test_admm_position_controlled_form_dense_weights(amd, variant):
    """The position-controlled form of the bounded QP (planar hand, cost on du = u_t - u_{t-1}, alpha_R = 1) with a
    Q that mixes object and finger coordinates and a dense R: KKT-certified on the augmented statement, and equal
    to the oracle's ADMM."""
    a = _admm_du_problem()
    T, idx, rows = a["T"], a["idx"], a["rows"]
    assert a["it"] < 40000 and max(a["res"]) < 1e-5, (a["it"], a["res"])

    def run(v):
        Q, Qd, R = spelled(a, v)
        return amd.solve_tvlqr(a["A"], a["B"], a["c"], Q, Qd, R, a["x0"], a["xd"], None, indices_u_into_x=idx,
                               u_bound_abs=np.stack([rows[2], rows[3]]), u_bound_rel=np.stack([rows[4], rows[5]]),
                               rho=100.0, eps=1e-10, max_iter=40000)

    xs, us = run(variant)
    d = np.diff(np.vstack([a["x0"][idx][None], us]), axis=0)
    assert np.abs(d).max() > 0.03 - 1e-6 or np.abs(us - rows[2]).min() < 1e-6 or np.abs(us - rows[3]).min() < 1e-6
    Ab, Bb, cb, Qb, Qdb, xdb, z0, zlo, zhi = a["aug"]
    zx = np.hstack([xs, np.vstack([a["x0"][idx][None], us])])
    res = orc.qp_box_kkt_residuals(Ab, Bb, cb, Qb, Qdb, a["R"], z0, xdb, zlo, zhi, rows[4], rows[5], zx, d, alpha_R=1.0)
    print("KKT residuals (dynamics, box, stationarity, multiplier sign):", res)
    assert max(res) < 1e-5, res
    report("x* vs oracle ADMM", xs, a["zx"][:, :7], rtol=0, atol=1e-7)
    report("u* vs oracle ADMM", us, a["zx"][1:, 7:], rtol=0, atol=1e-7)
    if variant != "sym":
        x0s, u0s = run("sym")
        report("u*, %s vs symmetric part" % variant, us, u0s, **SAME)
        report("x*, %s vs symmetric part" % variant, xs, x0s, **SAME)


# ---------------------------------------------------------------- B2 / B3: the active-set descents
@functools.lru_cache(maxsize=None)
def _active_set_problem(seed):
    """test_quasistatic_active_set_random_problems' randomised planar-hand problem with diag(q) replaced by
    V diag(q) V' and a dense SPD R, and the oracle's descents (both kinds of bound)."""
    rng = np.random.default_rng(100 + seed)
    T = int(rng.integers(12, 30))
    sys_o, x0 = _hand_start()
    idx = sys_o.indices_u_into_x
    u_trj = np.tile(x0[HAND_IDX], (T, 1)) + 0.03 * rng.normal(size=(T, 4)).cumsum(axis=0) / np.sqrt(T)
    x_trj = orc.rollout(sys_o, x0, u_trj)
    du = 0.1 * rng.normal(size=(T, 300, 4))
    At, Bt, ct = orc.zero_order_B_decoupled(sys_o, x_trj, u_trj, du)
    q = HAND_Q * rng.uniform(0.3, 3.0, size=7)
    Q, Qd, R = _hand_weights(rng, q, rng.uniform(10, 200), rng.uniform(0.5, 10, size=4))
    xd = np.tile(x0 + HAND.pack(np.concatenate([rng.uniform(-0.3, 0.3, 2), rng.uniform(-0.6, 0.6, 1)]), [0, 0], [0, 0]),
                 (T + 1, 1))
    w = rng.uniform(0.01, 0.08)
    sol = {}
    for kind in ("abs", "rel"):
        ub = np.array([-np.ones(4) * w, np.ones(4) * w]) if kind == "abs" else None
        rb = np.array([-np.ones(4) * w, np.ones(4) * w]) if kind == "rel" else None
        rows = orc.quasistatic_bounds(x_trj, idx, None, ub, rb)
        lo, hi = (rows[2], rows[3]) if kind == "abs" else (rows[4], rows[5])
        xa, ua, stats = orc.local_descent_quasistatic_as(sys_o, At, Bt, ct, Q, Qd, R, x0, xd, lo, hi, kind)
        sol[kind] = (lo, hi, xa, ua, stats)
    return dict(T=T, idx=idx, x0=x0, At=At, Bt=Bt, ct=ct, Q=Q, Qd=Qd, R=R, xd=xd, sol=sol,
                unsym=unsym_of(Q, Qd, R, 200 + seed))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_active_set_descents_dense_weights(amd, seed, as_solver, variant):
    from irs_mpc_amd import device as dev
    a = _active_set_problem(seed)
    dm = amd.PlanarHandDynamics(0.1).dm()
    assert np.abs(a["Q"][0, 1:]).max() > 1e-2                    # object and finger coordinates are mixed
    for kind in ("abs", "rel"):
        lo, hi, xa, ua, stats = a["sol"][kind]
        assert all(st[1] >= 0 for st in stats)
        kw = dict(u_lo=dev.to_dev(lo), u_hi=dev.to_dev(hi)) if kind == "abs" else \
            dict(du_lo=dev.to_dev(lo), du_hi=dev.to_dev(hi))

        def run(v):
            o = dm.quasistatic_box_descent(*[dev.to_dev(b) for b in (a["At"], a["Bt"], a["ct"], *spelled(a, v),
                                                                      a["xd"], a["x0"])],
                                           solver=as_solver, max_iter=2000, eps=1e-10, **kw)
            info = npy(o["info"])
            assert info[0] == 0 and info[2] == 0, (kind, v, info)
            return npy(o["u_new"]), npy(o["x_new"]), float(o["cost"].item())

        u, x, c = run(variant)
        report(kind + " u_new vs oracle", u, ua, rtol=0, atol=1e-8)
        report(kind + " x_new vs oracle", x, xa, rtol=0, atol=1e-8)
        report(kind + " cost", c, orc.eval_cost_quasistatic(x, u, a["xd"], a["Q"], a["Qd"], a["R"], a["idx"]), rtol=1e-12)
        if variant != "sym":
            us, xs, cs = run("sym")
            report("%s u_new, %s vs symmetric part" % (kind, variant), u, us, **SAME)
            report("%s x_new, %s vs symmetric part" % (kind, variant), x, xs, **SAME)
            report("%s cost, %s vs symmetric part" % (kind, variant), c, cs, **SAME)


# ---------------------------------------------------------------- B2 / B3: the CEM cost kernels
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name,h,T,std", hp.CEM_CASES, ids=[c[0] for c in hp.CEM_CASES])
def test_cem_rollout_costs_dense_weights(amd, name, h, T, std, variant):
    """irs_cem_rollout_costs against the oracle's costs of the same candidates (tvlqr_highprec.cem_candidates:
    open-loop rollouts the oracle itself is not sensitive to, tests/test_tvlqr_reference_cpu.py)."""
    from irs_mpc_amd import device as dev
    p = hp.model_problem(name, h, T)
    dm = _device_system(amd, name, h).dm()
    cand, want = hp.cem_candidates(name, h, T, std)

    def run(v):
        Q, _, R = spelled(p, v)
        return npy(dm.cem_rollout_costs(dev.to_dev(cand), dev.to_dev(p["x0"]), dev.to_dev(Q), dev.to_dev(R),
                                        dev.to_dev(p["xd"])))

    got = run(variant)
    report("cem_rollout_costs", got, want, rtol=1e-12)
    if variant != "sym":
        report("cem_rollout_costs, %s vs symmetric part" % variant, got, run("sym"), **SAME)


def cem_quasistatic_costs(cand):
    """The oracle's quasistatic cost (du input cost, terminal Qd) of planar-hand candidates under the dense weights
    of _admm_du_problem."""
    a = _admm_du_problem()
    sys_o, x0 = _hand_start()
    return np.array([orc.eval_cost_quasistatic(orc.rollout(sys_o, x0, u), u, a["xd"], a["Q"], a["Qd"], a["R"], a["idx"])
                     for u in cand])


@functools.lru_cache(maxsize=None)
def cem_quasistatic_candidates(B=24):
    a = _admm_du_problem()
    _, x0 = _hand_start()
    cand = np.tile(x0[HAND_IDX], (B, a["T"], 1)) + 0.05 * np.random.default_rng(11).normal(size=(B, a["T"], 4))
    return cand, cem_quasistatic_costs(cand)


@pytest.mark.parametrize("variant", VARIANTS)
def test_cem_rollout_costs_quasistatic_dense_weights(amd, variant):
    from irs_mpc_amd import device as dev
    a = _admm_du_problem()
    _, x0 = _hand_start()
    dm = amd.PlanarHandDynamics(0.1).dm()
    cand, want = cem_quasistatic_candidates()

    def run(v):
        Q, Qd, R = spelled(a, v)
        return npy(dm.cem_rollout_costs_quasistatic(dev.to_dev(cand), dev.to_dev(x0), dev.to_dev(Q), dev.to_dev(Qd),
                                                    dev.to_dev(R), dev.to_dev(a["xd"])))

    got = run(variant)
    report("cem_rollout_costs_quasistatic", got, want, rtol=1e-12)
    if variant != "sym":
        report("cem_rollout_costs_quasistatic, %s vs symmetric part" % variant, got, run("sym"), **SAME)


# ---------------------------------------------------------------- B2 / B3: the fused iterate
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name,cls,N,iters,T", [("pendulum", "IrsLqrExact", 0, 3, 40),
                                               ("quadrotor", "IrsLqrFirstOrder", 400, 2, 20)],
                         ids=["pendulum-exact", "quadrotor-first-order"])
def test_fused_iterate_dense_weights_equals_the_host_loop(amd, name, cls, N, iters, T, variant, capsys):
    """IrsLqr.iterate through one library call == the host loop, bit for bit (test_fused_iterate_equals_the_host_loop's
    pattern), with dense weights; and an unsymmetric spelling walks the same trajectories as its symmetric part."""
    from examples.problems import PROBLEMS
    h = 0.05
    w = hp.model_problem(name, h, {"pendulum": 30, "quadrotor": 20}[name])      # its weights; the problem is the example's

    def make(verbose, v):
        sysd, params, sm, _, _ = PROBLEMS[name](T)
        params.Q, params.Qd, params.R = spelled(w, v)
        if cls == "IrsLqrExact":
            sol = amd.IrsLqrExact(sysd, params)
        else:
            sol = getattr(amd, cls)(sysd, params, amd.GaussianSmoothing(sm["std_x"], sm["std_u"], N, power=sm["power"],
                                                                       seed=5))
        sol.verbose = verbose
        return sol

    a, b = make(False, variant), make(True, variant)
    a.iterate(iters)
    b.iterate(iters)
    capsys.readouterr()
    assert len(a.cost_lst) == len(b.cost_lst) == iters + 2
    assert np.isfinite(a.cost_lst).all()
    np.testing.assert_array_equal(np.array(a.cost_lst), np.array(b.cost_lst))
    for xa, xb in zip(a.x_trj_lst, b.x_trj_lst):
        np.testing.assert_array_equal(xa, xb)
    for ua, ub in zip(a.u_trj_lst, b.u_trj_lst):
        np.testing.assert_array_equal(ua, ub)
    # the initial cost is the oracle's evaluate_cost of the oracle's rollout, dense Q and R
    sys_o = orc.SYSTEMS[name](h)
    _, params, _, _, _ = PROBLEMS[name](T)
    x_init = orc.rollout(sys_o, params.x0, params.u_trj_initial)
    report("initial cost", a.cost_lst[0], orc.evaluate_cost(x_init, params.u_trj_initial, params.xd_trj, w["Q"], w["R"]),
           rtol=1e-12)
    if variant != "sym":
        s = make(False, "sym")
        s.iterate(iters)
        report("cost history, %s vs symmetric part" % variant, a.cost_lst, s.cost_lst, **SAME)
        for i, (xa, xs) in enumerate(zip(a.x_trj_lst, s.x_trj_lst)):
            report("x_trj[%d], %s vs symmetric part" % (i, variant), xa, xs, **SAME)
        for i, (ua, us) in enumerate(zip(a.u_trj_lst, s.u_trj_lst)):
            report("u_trj[%d], %s vs symmetric part" % (i, variant), ua, us, **SAME)
