"""Admission of the verdict cases (tests/helpers/verdict_cases.py) by the extended-precision pivot trace
(oracle/tvlqr_highprec.py: pivot_trace), and the trace itself against the references it extends.

The admission is a condition, not a measurement: a V1 case is used only if, in np.longdouble, the backward sweep's
Hessians H_t are positive definite for every t > t* with lambda_min(H_t) > 1e-6 max|H_t|, and H_{t*} is indefinite with
lambda_min(H_{t*}) < -1e-6 max|H_{t*}| (f64 eigvalsh of the longdouble H).  The margins are ten decades above f64
rounding, so the device's verdict cannot hinge on the order in which a kernel factors H.  Every case of the fixed lists
is asserted -- none is filtered -- and the lists' lengths are asserted too.
"""
import numpy as np
import pytest

from oracle import irs_oracle as orc
from oracle import tvlqr_highprec as hp
from tests.helpers import verdict_cases as vc

ADMM_DIRECTIONS = ("e0", "e1")        # the bounded control (sized against rho/2) and the unbounded one


def show(label, t_bad, margins, t_star):
    good = [margins[t] for t in margins if t != t_bad]
    print("%-58s t_bad %s  min good margin %s  margin at t* %s" % (
        label, t_bad, "%.3g" % min(good) if good else "-", "%.3g" % margins[t_star] if t_star is not None else "-"))


def admit(label, p, t_star, **pen):
    t_bad, margins = vc.trace(p, **pen)
    show(label, t_bad, margins, t_star)
    assert vc.admitted(t_bad, margins, t_star, p["T"]), (label, t_bad, margins)


# ---------------------------------------------------------------------------------------------- the trace itself
def test_pivot_trace_is_the_riccati_reference_on_a_healthy_problem():
    """On the dense conformance problem the trace finds every Hessian positive definite, and its H_t is alpha R + B'PB
    of the P the gain recursion of tvlqr_riccati carries: K_t = -H_t^-1 B_t'P A_t reproduces the reference's gains."""
    n, m, T = 5, 2, 8
    p = hp.riccati_problem(n, m, T, "spd")
    t_bad, H = hp.pivot_trace(p["At"], p["Bt"], p["Q"], p["Qd"], p["R"], 0.5)
    assert t_bad is None and sorted(H) == list(range(T))
    K, _ = hp.riccati_reference(n, m, T, "spd")
    # H_{T-1} = alpha R + B'Qd B, and K_{T-1} from it
    B, A = np.asarray(p["Bt"][T - 1], hp.LD), np.asarray(p["At"][T - 1], hp.LD)
    want = hp.LD(0.5) * hp.sym(p["R"]) + B.T.dot(hp.sym(p["Qd"])).dot(B)
    assert float(np.abs(H[T - 1] - want).max()) < 1e-17 * float(np.abs(want).max())
    Kt = -hp.cho_solve(hp.cholesky(H[T - 1]), B.T.dot(hp.sym(p["Qd"])).dot(A))
    assert hp.within(Kt, K[T - 1], frac=1e-6) <= 1.0
    # and one step on, through P_{T-1}: the trace's H_{T-2} against the oracle's f64 recursion
    Ko, _ = orc.tvlqr_riccati(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["xd"])
    Acl = p["At"][T - 1] + p["Bt"][T - 1].dot(Ko[T - 1])
    P1 = p["Q"] + p["At"][T - 1].T.dot(p["Qd"]).dot(Acl)
    H2 = 0.5 * p["R"] + p["Bt"][T - 2].T.dot(0.5 * (P1 + P1.T)).dot(p["Bt"][T - 2])
    np.testing.assert_allclose(np.asarray(H[T - 2], float), H2, rtol=1e-12)


def test_pivot_trace_stops_at_the_first_indefinite_step_and_names_the_pivot():
    """The sweep stops where the Cholesky factorisation fails, and with the negative direction along e_j it fails at
    pivot j + 1 -- the position a kernel's LDL' meets it at."""
    n, m, T = 7, 4, 8
    for j in range(m):
        c = vc.plain_case(n, m, T, T // 2, "e%d" % j)
        t_bad, H = hp.pivot_trace(c["At"], c["Bt"], c["Q"], c["Qd"], c["R"], 0.5)
        assert t_bad == T // 2 and sorted(H) == list(range(T // 2, T))
        with pytest.raises(np.linalg.LinAlgError, match="pivot %d" % (j + 1)):
            hp.cholesky(H[t_bad])


def test_the_two_spellings_of_the_position_controlled_qp_have_the_same_hessians():
    """Control du on [A B; 0 I] and control u with the stage cross term [0; -R]: one problem, so the same H_t -- and
    both are the H of the oracle's active-set sweep (orc.ctrlbox_backward) on the empty active set."""
    c = vc.du_healthy("planar_hand")
    p = vc.problem_of(c, 1)
    T, m = p["T"], p["R"].shape[0]
    out = {}
    for control in ("du", "abs"):
        f = hp.position_controlled_form(p["At"], p["Bt"], p["Q"], p["Qd"], p["R"], control)
        t_bad, out[control] = hp.pivot_trace(f["At"], f["Bt"], f["Q"], f["Qd"], f["R"], 1.0, cross=f["cross"])
        assert t_bad is None
    for kind, control in (("rel", "du"), ("abs", "abs")):
        prob = orc.quasistatic_ctrl_problem(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["xd"], kind)
        W = orc.ctrlbox_workspace(prob)
        act = np.zeros((T, m))
        big = np.full((T, m), 1e9)
        orc.ctrlbox_backward(prob, act, -big, big, T - 1, 0, W)
        for t in range(T):
            np.testing.assert_allclose(np.asarray(out[control][t], float), W["H"][t], rtol=1e-10, atol=1e-12)
    for t in range(T):
        d = np.abs(out["du"][t] - out["abs"][t]).max() / np.abs(out["du"][t]).max()
        assert float(d) < 1e-15, (t, float(d))


def test_penalised_weights_are_those_of_the_admm_factorisation():
    """half_rho, pen_x, pen_u: H_{T-1} = alpha R + rho/2 Mu + B'(Qd + rho/2 Mx)B (csrc/boxqp_factor.inc), and the
    oracle's ADMM factor (orc.tvlqr_box_factor) inverts exactly these Hessians."""
    n, m, T = 3, 2, 9
    p = hp.riccati_problem(n, m, T, "spd")
    rho = 0.7
    xlo, xhi = np.array([-np.inf, -5.0, -np.inf]), np.array([np.inf, 5.0, np.inf])
    ulo, uhi = np.array([-3.0, -np.inf]), np.array([3.0, np.inf])
    t_bad, H = hp.pivot_trace(p["At"], p["Bt"], p["Q"], p["Qd"], p["R"], 0.5, half_rho=0.5 * rho, pen_x=[0, 1, 0],
                              pen_u=[1, 0])
    assert t_bad is None
    B = p["Bt"][T - 1]
    want = 0.5 * p["R"] + np.diag([0.5 * rho, 0.0]) + B.T.dot(p["Qd"] + np.diag([0.0, 0.5 * rho, 0.0])).dot(B)
    np.testing.assert_allclose(np.asarray(H[T - 1], float), want, rtol=1e-14)
    F = orc.tvlqr_box_factor(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], xlo, xhi, ulo, uhi, rho, alpha_R=0.5)
    for t in (0, T // 2, T - 1):
        np.testing.assert_allclose(F["Hinv"][t].dot(np.asarray(H[t], float)), np.eye(m), rtol=0, atol=1e-10)


# ---------------------------------------------------------------------------------------------- admission, V1
def test_plain_cases_are_admitted():
    count = 0
    for n, m, T, impl in vc.RICCATI_PATHS:
        for ts in vc.t_stars(T):
            for d in vc.directions(m):
                admit("riccati %s n%d m%d T%d t*%d %s" % (impl, n, m, T, ts, d), vc.plain_case(n, m, T, ts, d), ts)
                count += 1
    assert count == 3 * (1 + 3 + 5 + 5 + 5 + 3 + 5)


def test_descent_cases_are_admitted_and_their_neighbours_are_healthy():
    count = 0
    for name, h, T, impl in vc.DESCENT_PATHS:
        m = hp.model_problem(name, h, T)["Bt"].shape[2]
        for ts in vc.t_stars(T):
            for d in vc.directions(m):
                c = vc.descent_case(name, h, T, ts, d)
                for b in range(3):
                    admit("descent %s %s T%d t*%d %s problem %d" % (name, impl, T, ts, d, b), vc.problem_of(c, b),
                          ts if b == c["bad"] else None)
                count += 1
    assert count == 3 * (1 + 3 + 5 + 5)


def test_admm_cases_are_admitted():
    count = 0
    for ts in vc.t_stars(vc.ADMM_MODEL[2]):
        for d in ADMM_DIRECTIONS:
            c = vc.admm_case(ts, d)
            pen = dict(half_rho=0.5 * c["rho"], pen_x=c["pen_x"], pen_u=c["pen_u"])
            for b in range(3):
                admit("admm bicycle t*%d %s problem %d" % (ts, d, b), vc.problem_of(c, b), ts if b == c["bad"] else None,
                      **pen)
            count += 1
    for ts in vc.t_stars(vc.VALUES_SIZE[2]):
        for d in ADMM_DIRECTIONS:
            c = vc.values_case(ts, d)
            admit("box_values n%d m%d T%d t*%d %s" % (*vc.VALUES_SIZE, ts, d), c, ts, half_rho=0.5 * c["rho"],
                  pen_x=c["pen_x"], pen_u=c["pen_u"])
            count += 1
    assert count == 12


def test_position_controlled_cases_are_admitted():
    """Per model, t*, failing pivot j and kind of box: the ADMM's penalised Hessians (solver 1) and the active-set
    solvers' plain ones (2, 3, the batch), the latter in both spellings."""
    count = 0
    for model in vc.DU_MODELS:
        m = len(vc.du_start(model)[2])
        for ts in vc.t_stars(vc.DU_T):
            for j in range(m):
                c = vc.du_case(model, ts, j)
                for b in range(3):
                    p, want = vc.problem_of(c, b), (ts if b == c["bad"] else None)
                    for kind, control in (("abs", "abs"), ("rel", "du")):
                        for solver in (1, 2):
                            pen_x, pen_u = vc.du_penalties(c, kind, solver)
                            # the ADMM factors the du spelling under either box
                            t_bad, margins = vc.trace_du(p, "du" if solver == 1 else control, 0.5 * c["rho"], pen_x, pen_u)
                            if b == c["bad"]:
                                show("%s t*%d pivot %d %s solver %s" % (model, ts, j + 1, kind, "1" if solver == 1 else "2/3"),
                                     t_bad, margins, ts)
                            assert vc.admitted(t_bad, margins, want, p["T"]), (model, ts, j, b, kind, solver, t_bad, margins)
                count += 1
    assert count == 3 * (2 + 4)


def test_position_controlled_cases_fail_at_the_planted_pivot():
    """Column j of B_{t*} carries the concave cost: the closed-form inverse of csrc/ctrlbox_mfma.hip meets the negative
    pivot at position j + 1 (p, det, the Schur block's p, its det) -- every position is covered."""
    for model in vc.DU_MODELS:
        m = len(vc.du_start(model)[2])
        for j in range(m):
            c = vc.du_case(model, vc.DU_T // 2, j)
            p = vc.problem_of(c, c["bad"])
            f = hp.position_controlled_form(p["At"], p["Bt"], p["Q"], p["Qd"], p["R"], "du")
            t_bad, H = hp.pivot_trace(f["At"], f["Bt"], f["Q"], f["Qd"], f["R"], 1.0)
            with pytest.raises(np.linalg.LinAlgError, match="pivot %d" % (j + 1)):
                hp.cholesky(H[t_bad])


# ---------------------------------------------------------------------------------------------- admission, V2
def test_healthy_twins_are_positive_definite_throughout():
    """The problems V2 poisons: every Hessian positive definite by the margin, so a non-zero verdict on the poisoned
    copy is the poison's doing."""
    for n, m, T, impl in vc.RICCATI_PATHS:
        admit("healthy riccati %s n%d m%d T%d" % (impl, n, m, T), vc.healthy_plain(n, m, T), None)
    for name, h, T, impl in vc.DESCENT_PATHS:
        c = vc.healthy_descent(name, h, T)
        for b in range(3):
            admit("healthy descent %s T%d problem %d" % (name, T, b), vc.problem_of(c, b), None)
    c = vc.healthy_admm()
    for b in range(3):
        admit("healthy admm problem %d" % b, vc.problem_of(c, b), None, half_rho=0.5 * c["rho"], pen_x=c["pen_x"],
              pen_u=c["pen_u"])
    c = vc.healthy_values()
    admit("healthy box_values", c, None, half_rho=0.5 * c["rho"], pen_x=c["pen_x"], pen_u=c["pen_u"])
    for model in vc.DU_MODELS:
        c = vc.du_healthy(model)
        for b in range(3):
            for kind, control in (("abs", "abs"), ("rel", "du")):
                for solver in (1, 2):
                    pen_x, pen_u = vc.du_penalties(c, kind, solver)
                    t_bad, margins = vc.trace_du(vc.problem_of(c, b), "du" if solver == 1 else control, 0.5 * c["rho"],
                                                 pen_x, pen_u)
                    assert vc.admitted(t_bad, margins, None, c["T"]), (model, b, kind, solver, t_bad, margins)


def test_poisoned_copies_differ_from_their_problem_in_one_element():
    c = vc.healthy_descent("bicycle", 0.1, 8)
    p = vc.problem_of(c, 1)
    for field in vc.FIELDS:
        for poison in vc.POISONS:
            q = vc.poisoned(p, field, poison)
            diff = ~np.isfinite(q[field])
            assert diff.sum() == 1 and np.isfinite(p[field]).all()
            for other in vc.FIELDS:
                if other != field:
                    assert q[other] is p[other]
            cb = vc.poisoned_batch(c, field, poison)
            bad_rows = [b for b in range(3) if not np.isfinite(cb["batch"][field][b]).all()]
            assert bad_rows == [1] and np.isfinite(c["batch"][field]).all()
