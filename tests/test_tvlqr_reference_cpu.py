"""The extended-precision TV-LQR reference (oracle/tvlqr_highprec.py) pinned on the CPU, and the admission
check of every input the GPU conformance tests (tests/test_tvlqr_dense_gpu.py) use: on each of them the f64
oracle has to stay within 1/100 of the device tolerance of the extended-precision answer, so that a mismatch on
the device is a fault of the device code and not an ill-conditioned problem."""
import numpy as np
import pytest

from oracle import irs_oracle as orc
from oracle import tvlqr_highprec as hp

CASE_IDS = ["n%d-m%d-T%d-%s" % c for c in hp.RICCATI_CASES]


@pytest.mark.parametrize("n,m,T", [(5, 2, 6), (2, 1, 9), (3, 16, 4), (12, 4, 5)])
def test_reference_plan_equals_the_kkt_solution(n, m, T):
    """Backward pass + linear rollout == the literal KKT statement of the reference's QP (an independent
    method: one dense symmetric indefinite solve, no recursion), dense SPD weights."""
    p = hp.riccati_problem(n, m, T, "spd")
    x, u = hp.solve_tvlqr(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["x0"], p["xd"])
    xq, uq = orc.solve_tvlqr_qp(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["x0"], p["xd"])
    ex, eu = hp.within(xq, x, 0.01), hp.within(uq, u, 0.01)
    print("KKT vs extended precision, in units of 1/100 of the device tolerance: x %.3g u %.3g" % (ex, eu))
    assert ex <= 1.0 and eu <= 1.0


@pytest.mark.parametrize("family", hp.FAMILIES)
@pytest.mark.parametrize("n,m,T,impl", hp.RICCATI_CASES, ids=CASE_IDS)
def test_f64_oracle_within_a_hundredth_of_the_device_tolerance(n, m, T, impl, family):
    p = hp.riccati_problem(n, m, T, family)
    for W in (p["Q"], p["Qd"], p["R"]):
        np.testing.assert_array_equal(W, W.T)
        assert np.abs(W).max() < 2.0 ** 11                      # what on_grid's exactness argument needs
    assert np.linalg.eigvalsh(p["R"]).min() > 0
    assert np.linalg.eigvalsh(p["Q"]).min() > -1e-8 and np.linalg.eigvalsh(p["Qd"]).min() > -1e-8
    if family == "psd_null" and n >= 2:
        assert np.linalg.eigvalsh(p["Q"])[0] < 1e-8              # the null space is there (to the grid)
    if family != "spd" and n >= 2:
        assert np.abs(p["Q"] - np.diag(np.diag(p["Q"]))).max() > 1e-3       # and the matrix is dense
    K, k = hp.riccati_reference(n, m, T, family)
    Ko, ko = orc.tvlqr_riccati(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["xd"], alpha_R=0.5)
    eK, ek = hp.within(Ko, K, 0.01), hp.within(ko, k, 0.01)
    print("f64 oracle vs extended precision, units of 1/100 of the device tolerance: K %.3g k %.3g" % (eK, ek))
    assert eK <= 1.0 and ek <= 1.0


@pytest.mark.parametrize("n,m,T", [(2, 1, 30), (5, 2, 40), (3, 16, 9), (12, 4, 50)])
def test_reference_uses_the_symmetric_part(n, m, T):
    """The contract: weights need not be symmetric, the symmetric part is used.  On the grid the symmetric part
    of the unsymmetric spellings is the symmetric weight exactly, so the answers are identical; off the grid they
    agree to the rounding of (s + k) + (s - k).  And the effect is not small: the f64 oracle, which does not
    symmetrise, moves K by far more than any tolerance here."""
    p = hp.riccati_problem(n, m, T, "spd")
    K, k = hp.riccati_reference(n, m, T, "spd")
    for name, (Q, Qd, R) in p["unsym"].items():
        assert np.abs(Q - Q.T).max() > 0.05
        np.testing.assert_array_equal(0.5 * (Q + Q.T), p["Q"])
        np.testing.assert_array_equal(0.5 * (R + R.T), p["R"])
        K2, k2 = hp.tvlqr_riccati(p["At"], p["Bt"], p["ct"], Q, Qd, R, p["xd"])
        np.testing.assert_array_equal(K2, K, err_msg=name)
        np.testing.assert_array_equal(k2, k, err_msg=name)
    rng = np.random.default_rng(5)
    S, Sm = rng.normal(size=(n, n)), rng.normal(size=(m, m))
    K3, k3 = hp.tvlqr_riccati(p["At"], p["Bt"], p["ct"], p["Q"] + 0.3 * (S - S.T), p["Qd"] + 0.3 * (S - S.T),
                              p["R"] + 0.3 * (Sm - Sm.T), p["xd"])
    assert hp.within(K3, K, 1e-4) <= 1.0 and hp.within(k3, k, 1e-4) <= 1.0
    if n > 1:
        Q, Qd, R = p["unsym"]["skew"]
        Ko, _ = orc.tvlqr_riccati(p["At"], p["Bt"], p["ct"], Q, Qd, R, p["xd"])
        assert hp.within(Ko, K) > 1e3


def test_cholesky_reports_an_indefinite_matrix():
    with pytest.raises(np.linalg.LinAlgError):
        hp.cholesky(np.array([[1.0, 2.0], [2.0, 1.0]]))
    A = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, 0.2], [0.5, 0.2, 2.0]])
    L = hp.cholesky(A)
    assert float(np.abs(L.dot(L.T) - A).max()) < 1e-17
    b = np.array([1.0, -2.0, 0.5])
    assert float(np.abs(A.astype(hp.LD).dot(hp.cho_solve(L, b)) - b).max()) < 1e-17


@pytest.mark.parametrize("name,h,T", hp.MODEL_CASES, ids=["%s-T%d" % (c[0], c[2]) for c in hp.MODEL_CASES])
def test_model_descent_inputs_are_well_conditioned(name, h, T):
    """The descents of the device models with dense weights: gains of the f64 oracle within 1/100 of the device
    tolerance of the reference, and the closed loop on the TRUE dynamics no more sensitive than that to which of
    the two sets of gains drives it."""
    p = hp.model_problem(name, h, T)
    K, k = hp.tvlqr_riccati(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["xd"])
    xo, uo, Ko, ko = orc.local_descent(p["sys_o"], p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["x0"], p["xd"])
    xr, ur = orc.closed_loop_rollout(p["sys_o"], K.astype(float), k.astype(float), p["x0"])
    figs = (hp.within(Ko, K, 0.01), hp.within(ko, k, 0.01), hp.within(xo, xr, 0.01), hp.within(uo, ur, 0.01))
    print("units of 1/100 of the device tolerance: K %.3g k %.3g x_new %.3g u_new %.3g" % figs)
    assert max(figs) <= 1.0
    assert np.isfinite(xo).all() and np.abs(xo - p["x_trj"]).max() < 10.0       # the closed loop stays by the nominal


def _ulp_sensitivity(costs_of, cand, want):
    """Largest relative change of the oracle's cost when every input moves to the next f64."""
    return float(np.abs(costs_of(np.nextafter(cand, np.inf)) / want - 1.0).max())


@pytest.mark.parametrize("name,h,T,std", hp.CEM_CASES, ids=[c[0] for c in hp.CEM_CASES])
def test_cem_candidates_are_well_conditioned(name, h, T, std):
    """The open-loop candidates of the CEM cost tests: one ulp on every input moves the oracle's own cost by no
    more than 1/100 of the rtol 1e-12 the device is held to."""
    p = hp.model_problem(name, h, T)
    cand, want = hp.cem_candidates(name, h, T, std)
    s = _ulp_sensitivity(lambda c: hp.open_loop_costs(p, c), cand, want)
    print("relative change of the cost under one ulp on the inputs: %.3g" % s)
    assert s <= 1e-14


def test_cem_quasistatic_candidates_are_well_conditioned():
    import test_tvlqr_dense_gpu as gpu_tests       # the planar-hand problem lives with its GPU tests
    cand, want = gpu_tests.cem_quasistatic_candidates()
    s = _ulp_sensitivity(gpu_tests.cem_quasistatic_costs, cand, want)
    print("relative change of the cost under one ulp on the inputs: %.3g" % s)
    assert s <= 1e-14
