"""The descents' verdicts on the device: which step a bad Hessian is reported at (V1), and never an all-clear on
non-finite data (V2) -- the two rules of include/irs_hip.h at every entry's `info`.

V1.  Every case of tests/helpers/verdict_cases.py has exactly one step t* whose control Hessian is not positive definite
in the backward sweep, admitted in extended precision by tests/test_descent_verdicts_cpu.py (margins 1e-6 max|H| on
either side of zero); each entry must report info[0] == t* + 1 -- for t* at the first step of the sweep, a middle one
and the last, for the failing pivot at every position, on every Riccati path at the smallest horizon that selects it,
and for the middle problem of a batch of three, whose neighbours keep the bits of their single calls.  (Q, Qd and R are
shared by a launch.  In the ADMM batch with the negative direction on the BOUNDED control, e0, the neighbours' own QP is
therefore concave inside the box too -- vc.admm_box -- and their verdicts are compared with their single calls' bits and
printed, not asserted clean; the ADMM batch case with a failing middle problem between neighbours asserted clean is e1.)

V2.  One NaN or +Inf at a mid-horizon step of At, Bt, ct, xd_trj, or in x0.  The healthy twin reports the all-clear (asserted
first: the poisoned verdict is then the poison's doing); the poisoned call reports 1 <= info[0] <= T + 1 (unbounded
entries) or info[0] != 0 or info[2] != 0 (bounded entries: the two words the host classes read).  In a batch the middle
problem is the poisoned one; its neighbours match their single calls bit for bit and report zeros.  One more element, row
0 of xd_trj, reaches nothing but the cost: the descents report T + 1 for it.

Non-finite data is no way to look for faults; before these cases ran, each kernel the poison reaches was read for three
things -- every loop it feeds is bounded by max_iter or T, no wait depends on a floating-point condition, and every
index chosen by a comparison stays in range when all comparisons are false:
  csrc/tvlqr.hip          backward pass and rollout loop over t only; no data-dependent index or wait.
  csrc/boxqp_kernel.inc,  the tail loop is `while (it < max_iter && !conv)`; the adaptive refactorisations are capped by
  csrc/boxqp_values.hip   max_refactor, the lazy ones by the set that only grows; every index is a function of (t, lane).
                          The residuals are fmax chains, which DROP a NaN: a poisoned tail could read "converged" -- the
                          bug these tests found (fixed: a tail whose first control is not finite has not converged).
  csrc/ctrlbox.hip        (:530-580) bq / wq start at 0x7fffffff and are dereferenced only behind `alpha < 1.0` /
                          `wmax > tol`; alpha = wave_min(best) and wmax = wave_max(worst) are never NaN (best / worst
                          move only through `room < best` / `viol > worst`, false on a NaN) and the lane that owns the
                          extremum holds a valid index.  All loops: kPdasIter, max_iter, T.  IEEE compares throughout.
  csrc/ctrlbox_mfma.hip   (:1041-1181) the same selections, but the unit is compiled with -fno-honor-nans, under which
                          `wm > 0.0`, `alpha < 1.0` or `wmax > tol` may be folded as if no operand were a NaN: the
                          sentinel could reach act_[] / backward_sweep.  Fixed before the first run: each selected index
                          is range-checked in integer arithmetic.  The clipping roll-out's chunk loop advances or stops.
  csrc/contact_models.hpp the plant's exact step QP: 3 repair rounds, 4 NC active-set steps, candidate indices that
                          default to row 0 and select by unrolled compares; no wait.
The two waves of the active-set kernels meet at workgroup barriers whose count depends on T alone.
"""
import numpy as np
import pytest
import torch

from tests.helpers import verdict_cases as vc

pytestmark = pytest.mark.gpu

LIN = ("At", "Bt", "ct")
ADMM_DIRECTIONS = ("e0", "e1")


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()     # fails loudly if the HIP library is missing
    return irs_mpc_amd


def D(a):
    from irs_mpc_amd import device as dev
    return dev.to_dev(np.ascontiguousarray(a, dtype=float))


def npy(t):
    return t.detach().cpu().numpy()


def same_bits(got, want, what):
    """Bit for bit: the raw words are compared, so +0 / -0 and two different NaNs count as different."""
    g, w = np.ascontiguousarray(npy(got)).reshape(-1), np.ascontiguousarray(npy(want)).reshape(-1)
    assert g.dtype == w.dtype and g.shape == w.shape, what
    bits = {8: np.int64, 4: np.int32}[g.dtype.itemsize]
    assert np.array_equal(g.view(bits), w.view(bits)), what


def device_model(amd, name, h):
    return {"pendulum": amd.PendulumDynamics, "bicycle": amd.BicycleDynamics, "quadrotor": amd.QuadrotorDynamics,
            "planar_hand": amd.PlanarHandDynamics, "box_pivoting": amd.BoxPivotingDynamics}[name](h).dm()


def ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


def unbounded_verdict(info, T):
    return 1 <= int(info) <= T + 1


def bounded_verdict(info):
    return info[0] != 0 or info[2] != 0


def planted(fields):
    return [(f, p) for f in fields for p in vc.POISONS]


# ================================================================================================ irs_tvlqr_riccati
def riccati(p):
    from irs_mpc_amd import device as dev
    _, _, info = dev.tvlqr_riccati(*[D(p[k]) for k in LIN], D(p["Q"]), D(p["Qd"]), D(p["R"]), D(p["xd"]),
                                   alpha_R=p["alpha_R"])
    return int(info.item())


@pytest.mark.parametrize("n,m,T,impl", vc.RICCATI_PATHS, ids=ids(vc.RICCATI_PATHS))
def test_riccati_reports_the_step(amd, n, m, T, impl):
    for ts in vc.t_stars(T):
        for d in vc.directions(m):
            info = riccati(vc.plain_case(n, m, T, ts, d))
            print("riccati %s t* %d %s: info %d" % (impl, ts, d, info))
            assert info == ts + 1, (impl, ts, d, info)


@pytest.mark.parametrize("n,m,T,impl", vc.RICCATI_PATHS, ids=ids(vc.RICCATI_PATHS))
def test_riccati_never_clean_on_nonfinite_data(amd, n, m, T, impl):
    p = vc.healthy_plain(n, m, T)
    assert riccati(p) == 0
    for field, poison in planted(("At", "Bt", "ct", "xd")):
        info = riccati(vc.poisoned(p, field, poison))
        print("riccati %s %s %s: info %d" % (impl, field, poison, info))
        assert unbounded_verdict(info, T), (impl, field, poison, info)


# ================================================================================================ irs_tvlqr_descent[_batch]
DESCENT_KEYS = ("K", "k", "x_new", "u_new", "cost", "info")


def descent_single(dm, p):
    return dm.tvlqr_descent(*[D(p[k]) for k in LIN], D(p["Q"]), D(p["Qd"]), D(p["R"]), D(p["xd"]), D(p["x0"]),
                            alpha_R=p["alpha_R"])


def descent_batch(dm, c):
    b = c["batch"]
    return dm.tvlqr_descent_batch(*[D(b[k]) for k in LIN], D(c["Q"]), D(c["Qd"]), D(c["R"]), D(b["xd"]), D(b["x0"]),
                                  alpha_R=c["alpha_R"])


@pytest.mark.parametrize("name,h,T,impl", vc.DESCENT_PATHS, ids=ids(vc.DESCENT_PATHS))
def test_descent_and_batch_report_the_step(amd, name, h, T, impl):
    dm = device_model(amd, name, h)
    m = dm.m
    for ts in vc.t_stars(T):
        for d in vc.directions(m):
            c = vc.descent_case(name, h, T, ts, d)
            got = descent_batch(dm, c)
            for b in range(3):
                one = descent_single(dm, vc.problem_of(c, b))
                for key in DESCENT_KEYS:
                    same_bits(got[key][b], one[key], (name, T, ts, d, b, key))
                info = int(one["info"].item())
                if b == c["bad"]:
                    print("descent %s %s t* %d %s: info %d" % (name, impl, ts, d, info))
                    assert info == ts + 1, (name, impl, ts, d, info)
                else:
                    assert info == 0 and np.isfinite(npy(one["x_new"])).all() and np.isfinite(float(one["cost"].item()))


@pytest.mark.parametrize("name,h,T,impl", vc.DESCENT_PATHS, ids=ids(vc.DESCENT_PATHS))
def test_descent_and_batch_never_clean_on_nonfinite_data(amd, name, h, T, impl):
    dm = device_model(amd, name, h)
    c = vc.healthy_descent(name, h, T)
    clean = [descent_single(dm, vc.problem_of(c, b)) for b in range(3)]
    for o in clean:
        assert int(o["info"].item()) == 0 and np.isfinite(float(o["cost"].item()))
    for field, poison in planted(vc.FIELDS):
        cb = vc.poisoned_batch(c, field, poison)
        got = descent_batch(dm, cb)
        one = descent_single(dm, vc.problem_of(cb, c["bad"]))
        info = int(one["info"].item())
        print("descent %s %s %s %s: info %d" % (name, impl, field, poison, info))
        assert unbounded_verdict(info, T), (name, field, poison, info)
        for b in range(3):
            want = one if b == c["bad"] else clean[b]
            for key in DESCENT_KEYS:
                same_bits(got[key][b], want[key], (name, field, poison, b, key))
    # row 0 of xd_trj reaches no gain: only the cost says so
    p = vc.problem_of(c, 1)
    p["xd"] = np.array(p["xd"], copy=True)
    p["xd"][0, 0] = np.nan
    assert int(descent_single(dm, p)["info"].item()) == T + 1


# ================================================================================================ irs_tvlqr_box_descent & co
BOX_ENTRIES = {"on_chip": dict(), "hbm_records": dict(records_in_hbm=True), "adaptive": dict(adaptive_rho=True),
               "lazy": dict(lazy_bounds=True)}


def box_single(dm, p, c, entry):
    n, m = dm.n, dm.m
    ulo, uhi = vc.admm_box(m)
    kw = dict(BOX_ENTRIES[entry])
    if entry == "lazy":
        kw["enforced"] = np.ones(n + m, dtype=np.int32)     # the penalty of the bounded control is in from the start
    return dm.tvlqr_box_descent(*[D(p[k]) for k in LIN], D(p["Q"]), D(p["Qd"]), D(p["R"]), D(p["xd"]), D(p["x0"]),
                                D(np.full(n, -np.inf)), D(np.full(n, np.inf)), D(ulo), D(uhi), alpha_R=p["alpha_R"],
                                rho=c["rho"], max_iter=vc.MAX_ITER, eps=vc.EPS, **kw)


def box_batch(dm, c):
    n, m = dm.n, dm.m
    b = c["batch"]
    ulo, uhi = vc.admm_box(m, 3)
    return dm.tvlqr_box_descent_batch(*[D(b[k]) for k in LIN], D(c["Q"]), D(c["Qd"]), D(c["R"]), D(b["xd"]), D(b["x0"]),
                                      D(np.full((3, n), -np.inf)), D(np.full((3, n), np.inf)), D(ulo), D(uhi),
                                      alpha_R=c["alpha_R"], rho=c["rho"], max_iter=vc.MAX_ITER, eps=vc.EPS)


@pytest.mark.parametrize("entry", list(BOX_ENTRIES) + ["batch"])
def test_box_descent_reports_the_step(amd, entry):
    name, h, T = vc.ADMM_MODEL
    dm = device_model(amd, name, h)
    for ts in vc.t_stars(T):
        for d in ADMM_DIRECTIONS:
            c = vc.admm_case(ts, d)
            if entry != "batch":
                info = npy(box_single(dm, vc.problem_of(c, c["bad"]), c, entry)["info"])
            else:
                got = box_batch(dm, c)
                for b in range(3):
                    one = box_single(dm, vc.problem_of(c, b), c, "on_chip")
                    for key in ("x_new", "u_new", "info"):
                        same_bits(got[key][b], one[key], (ts, d, b, key))
                    if b != c["bad"]:
                        i = npy(one["info"])
                        print("  neighbour %d: info %s, max |x_new| %.3g" % (b, i, np.abs(npy(one["x_new"])).max()))
                        if d == "e1":                    # (e0: the neighbours' own QP is concave, vc.admm_box)
                            assert i[0] == 0 and i[2] == 0, (ts, d, b, i)
                info = npy(got["info"])[c["bad"]]
            print("box descent %s t* %d %s: info %s" % (entry, ts, d, info))
            assert info[0] == ts + 1, (entry, ts, d, info)


@pytest.mark.parametrize("entry", list(BOX_ENTRIES) + ["batch"])
def test_box_descent_never_clean_on_nonfinite_data(amd, entry):
    name, h, T = vc.ADMM_MODEL
    dm = device_model(amd, name, h)
    c = vc.healthy_admm()
    clean = [box_single(dm, vc.problem_of(c, b), c, "on_chip" if entry == "batch" else entry) for b in range(3)]
    for o in clean:
        info = npy(o["info"])
        assert info[0] == 0 and info[2] == 0 and 1 <= info[1] < vc.MAX_ITER, info
    for field, poison in planted(vc.FIELDS):
        cb = vc.poisoned_batch(c, field, poison)
        if entry != "batch":
            info = npy(box_single(dm, vc.problem_of(cb, c["bad"]), c, entry)["info"])
        else:
            got = box_batch(dm, cb)
            one = box_single(dm, vc.problem_of(cb, c["bad"]), c, "on_chip")
            for b in range(3):
                want = one if b == c["bad"] else clean[b]
                for key in ("x_new", "u_new", "info"):
                    same_bits(got[key][b], want[key], (field, poison, b, key))
            info = npy(got["info"])[c["bad"]]
        print("box descent %s %s %s: info %s" % (entry, field, poison, info))
        assert bounded_verdict(info), (entry, field, poison, info)
    if entry == "on_chip":
        p = vc.problem_of(c, 1)
        p["xd"] = np.array(p["xd"], copy=True)
        p["xd"][0, 0] = np.nan          # reaches nothing but the cost
        info = npy(box_single(dm, p, c, entry)["info"])
        assert info[0] == T + 1, info


# ================================================================================================ irs_box_values_begin / _tail
def values_begin(p):
    from irs_mpc_amd import device as dev
    ulo, uhi = vc.admm_box(p["R"].shape[0])
    return dev.box_values_begin(*[D(p[k]) for k in LIN], D(p["Q"]), D(p["Qd"]), D(p["R"]), D(p["xd"]), u_lo=D(ulo),
                                u_hi=D(uhi), alpha_R=p["alpha_R"], rho=p["rho"])


def test_box_values_begin_reports_the_step(amd):
    for ts in vc.t_stars(vc.VALUES_SIZE[2]):
        for d in ADMM_DIRECTIONS:
            info = npy(values_begin(vc.values_case(ts, d))["info"])
            print("box_values_begin t* %d %s: info %s" % (ts, d, info))
            assert info[0] == ts + 1, (ts, d, info)


def test_box_values_never_clean_on_nonfinite_data(amd):
    from irs_mpc_amd import device as dev
    p = vc.healthy_values()
    T = p["T"]
    h = values_begin(p)
    dev.box_values_tail(h, 0, D(p["x0"]), max_iter=vc.MAX_ITER, eps=vc.EPS)
    info = npy(h["info"])
    assert info[0] == 0 and info[2] == 0 and 1 <= info[1] < vc.MAX_ITER, info
    for field, poison in planted(vc.FIELDS):
        q = vc.poisoned(p, field, poison)
        h = values_begin(q)
        begun = npy(h["info"]).copy()
        if field != "x0":               # the factorisation has seen the poison: its own word already says so
            assert 1 <= begun[0] <= T + 1, (field, poison, begun)
        dev.box_values_tail(h, 0, D(q["x0"]), max_iter=vc.MAX_ITER, eps=vc.EPS)
        info = npy(h["info"])
        print("box_values %s %s: after begin %s, after tail 0 %s" % (field, poison, begun, info))
        assert bounded_verdict(info), (field, poison, info)
        if field == "x0":               # only the tail sees the start state
            assert begun[0] == 0 and info[2] == 1, (begun, info)


# ================================================================================================ irs_quasistatic_box_descent
QS_KEYS = ("x_new", "u_new", "cost", "info")
QS_CASES = [(model, solver, kind) for model in vc.DU_MODELS for solver in (1, 2, 3, "batch") for kind in ("abs", "rel")]


def qs_rows(c, kind, b=None):
    lo, hi = c["rows"][kind]
    if b is not None:
        lo, hi = lo[b], hi[b]
    return dict(u_lo=D(lo), u_hi=D(hi)) if kind == "abs" else dict(du_lo=D(lo), du_hi=D(hi))


def qs_single(dm, c, b, kind, solver):
    p = vc.problem_of(c, b)
    return dm.quasistatic_box_descent(*[D(p[k]) for k in LIN], D(p["Q"]), D(p["Qd"]), D(p["R"]), D(p["xd"]), D(p["x0"]),
                                      solver=solver, rho=c["rho"], max_iter=vc.MAX_ITER, eps=vc.EPS, **qs_rows(c, kind, b))


def qs_batch(dm, c, kind):
    b = c["batch"]
    return dm.quasistatic_box_descent_batch(*[D(b[k]) for k in LIN], D(c["Q"]), D(c["Qd"]), D(c["R"]), D(b["xd"]),
                                            D(b["x0"]), max_iter=vc.MAX_ITER, eps=vc.EPS, **qs_rows(c, kind))


def qs_run(dm, c, kind, solver, clean=None):
    """info of the case's failing / poisoned problem through `solver`; the batch also proves that every problem has the
    bits of its single call (solver 3) -- `clean`: the neighbours' single calls where they are known already."""
    bad = c["bad"]
    if solver != "batch":
        return npy(qs_single(dm, c, bad, kind, solver)["info"])
    got = qs_batch(dm, c, kind)
    for b in range(3):
        one = clean[b] if clean is not None and b != bad else qs_single(dm, c, b, kind, 3)
        for key in QS_KEYS:
            same_bits(got[key][b], one[key], (c["model"], kind, b, key))
        if b != bad:
            i = npy(one["info"])
            assert i[0] == 0 and i[2] == 0, (c["model"], kind, b, i)
    return npy(got["info"])[bad]


@pytest.mark.parametrize("model,solver,kind", QS_CASES, ids=ids(QS_CASES))
def test_quasistatic_descent_reports_the_step(amd, model, solver, kind):
    dm = device_model(amd, model, 0.1)
    for ts in vc.t_stars(vc.DU_T):
        for j in range(dm.m):
            info = qs_run(dm, vc.du_case(model, ts, j), kind, solver)
            print("%s solver %s %s t* %d pivot %d: info %s" % (model, solver, kind, ts, j + 1, info))
            assert info[0] == ts + 1, (model, solver, kind, ts, j, info)


@pytest.mark.parametrize("model,solver,kind", QS_CASES, ids=ids(QS_CASES))
def test_quasistatic_descent_never_clean_on_nonfinite_data(amd, model, solver, kind):
    dm = device_model(amd, model, 0.1)
    c = vc.du_healthy(model)
    one = 3 if solver == "batch" else solver
    clean = [qs_single(dm, c, b, kind, one) for b in range(3)]
    for o in clean:
        info = npy(o["info"])
        assert info[0] == 0 and info[2] == 0 and np.isfinite(float(o["cost"].item())), info
    for field, poison in planted(vc.FIELDS):
        info = qs_run(dm, vc.poisoned_batch(c, field, poison), kind, solver, clean)
        print("%s solver %s %s %s %s: info %s" % (model, solver, kind, field, poison, info))
        assert bounded_verdict(info), (model, solver, kind, field, poison, info)
    if solver != "batch":
        cb = dict(c, batch={k: np.array(v, copy=True) for k, v in c["batch"].items()})
        cb["batch"]["xd"][c["bad"], 0, 0] = np.nan          # reaches nothing but the cost
        info = qs_run(dm, cb, kind, solver)
        assert info[0] == vc.DU_T + 1, (model, solver, kind, info)


# ================================================================================================ the host classes
def _pendulum_params(T, poison_row=None):
    from examples.problems import PROBLEMS
    sysd, params, _, _, _ = PROBLEMS["pendulum"](T)
    params.xbound = params.ubound = None
    params.xd_trj = np.array(params.xd_trj, float, copy=True)
    if poison_row is not None:
        params.xd_trj[poison_row, 0] = np.nan
    return sysd, params


@pytest.mark.parametrize("verbose", [False, True], ids=["fused-iterate", "host-loop"])
def test_irs_lqr_exact_raises_on_a_poisoned_goal(amd, verbose, capsys):
    """xd_trj with a NaN: the first descent's info is not zero and IrsLqrExact raises the reference's ValueError, on the
    fused path (one library call) and in the host loop alike, with nothing adopted."""
    T = 10
    sysd, params = _pendulum_params(T, poison_row=T // 2)
    sol = amd.IrsLqrExact(sysd, params)
    sol.verbose = verbose
    x_before = np.array(sol.x_trj, copy=True)
    with pytest.raises(ValueError, match="TV_LQR failed"):
        sol.iterate(3)
    capsys.readouterr()
    assert len(sol.cost_lst) == 1 and len(sol.x_trj_lst) == 1
    np.testing.assert_array_equal(sol.x_trj, x_before)
    # the same class on the clean goal runs
    sysd, params = _pendulum_params(T)
    ok = amd.IrsLqrExact(sysd, params)
    ok.verbose = verbose
    ok.iterate(3)
    capsys.readouterr()
    assert len(ok.cost_lst) == 5 and np.isfinite(ok.cost_lst).all()


def test_irs_lqr_quasistatic_raises_on_a_poisoned_goal(amd):
    from examples.run_quasistatic import problem
    T = 8

    def make(poison):
        q_dynamics, x0, u0, Q_dict, Qd_dict, R_dict, xd = problem(T, 0.1)
        p = amd.IrsLqrQuasistaticParameters()
        p.Q_dict, p.Qd_dict, p.R_dict = Q_dict, Qd_dict, R_dict
        xd = np.array(xd, float, copy=True)
        if poison:
            xd[T // 2, 0] = np.nan
        p.x0, p.x_trj_d, p.u_trj_0, p.T = x0, xd, u0, T
        p.u_bounds_abs = np.array([-np.ones(4) * 0.05, np.ones(4) * 0.05])
        p.sampling = lambda u_initial, it: u_initial / (it ** 0.8)
        p.std_u_initial, p.num_samples, p.publish_every_iteration = np.ones(4) * 0.1, 256, False
        p.device_rng_seed = 3
        return amd.IrsLqrQuasistatic(q_dynamics, p)

    bad = make(True)
    bad.verbose = False
    x_before = np.array(bad.x_trj, copy=True)
    with pytest.raises(ValueError, match="TV_LQR failed"):
        bad.iterate(2)
    np.testing.assert_array_equal(bad.x_trj, x_before)          # nothing was adopted
    ok = make(False)
    ok.verbose = False
    ok.iterate(2)
    assert np.isfinite(ok.cost)


def test_irs_lqr_batch_stops_the_poisoned_problem_alone(amd):
    """IrsLqrBatch, order "exact", three problems, the middle one with a NaN in its goal: it stops with the status any
    failed Riccati pass gets, and the other two walk, bit for bit, the trajectories of a batch without it."""
    from irs_mpc_amd.irs_lqr_batch import RICCATI_FAILED
    T = 10

    def params(b, poison):
        sysd, p = _pendulum_params(T, poison_row=T // 2 if poison else None)
        p.x0 = np.array([0.1 * b, 0.0])
        return sysd, p

    sysd = params(0, False)[0]
    three = amd.IrsLqrBatch(sysd, [params(0, False)[1], params(1, True)[1], params(2, False)[1]], "exact")
    two = amd.IrsLqrBatch(sysd, [params(0, False)[1], params(2, False)[1]], "exact")
    three.iterate(3)
    two.iterate(3)
    assert three.status[1] == RICCATI_FAILED and three.status[0] is None and three.status[2] is None
    assert two.status == [None, None]
    assert len(three.problems[1].cost_lst) == 1
    for b3, b2 in ((0, 0), (2, 1)):
        assert len(three.cost_lst[b3]) == len(two.cost_lst[b2]) == 5
        np.testing.assert_array_equal(np.array(three.cost_lst[b3]), np.array(two.cost_lst[b2]))
        for xa, xb in zip(three.x_trj_lst[b3], two.x_trj_lst[b2]):
            np.testing.assert_array_equal(xa, xb)
        for ua, ub in zip(three.u_trj_lst[b3], two.u_trj_lst[b2]):
            np.testing.assert_array_equal(ua, ub)
        assert np.isfinite(three.cost_lst[b3]).all()
