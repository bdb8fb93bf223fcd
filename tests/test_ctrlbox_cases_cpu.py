"""Admission of the active-set descent cases (oracle/ctrlbox_cases.py) that tests/test_ctrlbox_cases_gpu.py runs on
the two active-set kernels.  No GPU.

A case is admitted when the oracle loop (orc.local_descent_quasistatic_as on the oracle's contact dynamics) solves
it, every one of its T tails converges, every tail's candidate passes the solver-independent certificate
(ctrlbox_cases.tail_reference: box, stationarity, multiplier signs, relative to max |g|, below 1e-9) and the loop's
closed-loop control equals the certified first control to 1e-10.  And when it can show what it is for -- these are
conditions on the cases, not measurements:

  * every case but none / allinf has at least m first-control entries at a finite bound over the horizon (an entry
    with lo == hi is not counted: it binds whatever the kernel does);
  * every (model, kind) family has such entries at lo and at hi;
  * `gaps` has a finite bound that binds in an entry whose other side is infinite, a whole step and (m > 1) a whole
    component free on both sides; `pinned` has a lo == hi entry in a first row; `one_sided` has one infinite side
    per component;
  * `gaps` and `one_sided` at T >= 11 (the warm-start cases of the GPU file): at least half the entries of the first
    tail have a strict-complementarity margin above 1e-6;
  * each of the row-handling errors of mutated_rows (rows read one step late, row 0 broadcast, components reversed)
    moves some first control of the oracle loop by more than 1e-4 -- test_boxqp_cases_gpu.py's figure, and 1e4 x the
    1e-8 the device is held to.  Where an error changes no row (T = 1; m = 1 for the reversal) there is nothing to see.

Also here: the condensed statement the certificate is computed on and quasistatic_ctrl_problem's [x; w] rewrite give
the same cost for a random feasible plan.
"""
import numpy as np
import pytest

from oracle import ctrlbox_cases as cc
from oracle import irs_oracle as orc


@pytest.fixture(scope="module")
def admitted():
    """cid -> what admission found (filled by test_case_is_admitted, read by the family test after it)."""
    return {}


def bound_counts(c, cert):
    """(entries at a finite lo, at a finite hi) among the certified first controls, lo == hi entries left out."""
    both = c["lo"] == c["hi"]
    return int((cert["at_lo"] & ~both).sum()), int((cert["at_hi"] & ~both).sum())


@pytest.mark.parametrize("cid", list(cc.CASES))
def test_case_is_admitted(cid, admitted):
    c = cc.case(cid)
    T, m = c["T"], c["m"]
    assert c["lo"].shape == c["hi"].shape == (T, m) and (c["lo"] <= c["hi"]).all()
    x, u, stats = cc.oracle_descent(c)
    assert all(st[1] >= 0 for st in stats), stats                       # every tail of the loop converged
    cert = cc.certify_trajectory(c, x, u)
    assert cert["converged"] and cert["ok"], (cert["worst"], [r["res"] for r in cert["refs"]])
    err = np.abs(u - cert["u"]).max()
    n_lo, n_hi = bound_counts(c, cert)
    margins = cert["refs"][0]["margins"]
    strict = float((margins > 1e-6).mean())
    moved = {}
    for how in cc.MUTATIONS:
        rows = cc.mutated_rows(c, how)
        if rows is not None and cc.binds(c):
            moved[how] = np.abs(cc.oracle_descent(c, rows)[1] - u).max()
    print("%-24s residual %.1e  |u - certified| %.1e  at lo %d at hi %d of %d  strict %.2f  moved %s" % (
        cid, cert["worst"], err, n_lo, n_hi, u.size, strict, " ".join("%s %.1e" % kv for kv in moved.items())))
    assert err <= 1e-10, err
    admitted[cid] = (n_lo, n_hi)
    lo, hi = c["lo"], c["hi"]
    if not cc.binds(c):
        assert not np.isfinite(lo).any() and not np.isfinite(hi).any() and n_lo + n_hi == 0
        assert c["null"] == (c["shape"] == "none")
        return
    assert n_lo + n_hi >= m, (n_lo, n_hi)
    # |lo| != |hi| everywhere: the offsets of the two sides are independent draws
    fin = np.isfinite(c["off_lo"]) & np.isfinite(c["off_hi"]) & (c["off_lo"] != c["off_hi"])
    assert (np.abs(np.abs(c["off_lo"][fin]) - np.abs(c["off_hi"][fin])) > 1e-6).all()
    if c["shape"] == "ragged":
        assert np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()
    if c["shape"] == "one_sided":
        assert (np.isfinite(lo).all(axis=0) ^ np.isfinite(hi).all(axis=0)).all()
        assert (np.isfinite(lo).any(axis=0) ^ np.isfinite(hi).any(axis=0)).all()
    if c["shape"] == "gaps":
        free = ~np.isfinite(lo) & ~np.isfinite(hi)
        assert free.all(axis=1).any() and (m == 1 or free.all(axis=0).any())
        assert (cert["at_lo"] & ~np.isfinite(hi)).any() or (cert["at_hi"] & ~np.isfinite(lo)).any()
    if c["shape"] == "pinned":
        assert (lo[0] == hi[0]).any() and not (lo == hi).all()
    if c["shape"] == "offzero":
        centre = c["x_trj"][:-1, c["idx"]] if c["kind"] == "abs" else 0.0
        assert (((lo - centre) > 0) | ((hi - centre) < 0)).sum() >= m
    if c["shape"] in ("gaps", "one_sided") and T >= 11:
        assert strict >= 0.5, strict
    for how, d in moved.items():
        assert d > 1e-4, (how, d)
    if T >= 11:
        assert set(moved) == set(cc.MUTATIONS if m > 1 else cc.MUTATIONS[:2])


def test_every_family_binds_at_lo_and_at_hi(admitted):
    """Runs after the admissions above (file order) and reads their counts; a family admitted in part (a -k run) is
    recomputed."""
    for model in cc.MODELS:
        for kind in cc.KINDS:
            fam = [cid for cid, v in cc.CASES.items() if v[0] == model and v[1] == kind and v[2] in cc.BOUNDED]
            assert {cc.CASES[cid][2] for cid in fam} == set(cc.BOUNDED)
            assert {cc.CASES[cid][3] for cid in fam} == {1, 2, 11, 12}
            n_lo = n_hi = 0
            for cid in fam:
                if cid not in admitted:
                    c = cc.case(cid)
                    x, u, _ = cc.oracle_descent(c)
                    admitted[cid] = bound_counts(c, cc.certify_trajectory(c, x, u))
                n_lo, n_hi = n_lo + admitted[cid][0], n_hi + admitted[cid][1]
            print("%s-%s: at lo %d, at hi %d" % (model, kind, n_lo, n_hi))
            assert n_lo > 0 and n_hi > 0, (model, kind, n_lo, n_hi)
    shapes = {(v[0], v[1]): set() for v in cc.CASES.values()}
    for v in cc.CASES.values():
        shapes[(v[0], v[1])].add(v[2])
    assert all(s >= set(cc.BOUNDED) | {"allinf"} for s in shapes.values())
    assert all("none" in shapes[(model, "abs")] for model in cc.MODELS)


@pytest.mark.parametrize("cid", ["hand-abs-ragged-T11", "hand-rel-ragged-T12", "pivot-rel-gaps-T11",
                                 "push-abs-pinned-T12", "bob-abs-ragged-T2", "bob-rel-offzero-T11"])
def test_condensed_statement_equals_the_ctrl_problem(cid):
    """The cost of a random feasible plan of a tail, from a random state: the condensed original statement ==
    quasistatic_ctrl_problem's LQR in s = [x; w] rolled out stage by stage (rtol 1e-12)."""
    c = cc.case(cid)
    T, n, m, kind = c["T"], c["n"], c["m"], c["kind"]
    rng = np.random.default_rng(3)
    prob = orc.quasistatic_ctrl_problem(c["At"], c["Bt"], c["ct"], c["Q"], c["Qd"], c["R"], c["xd"], kind)
    for t in sorted({0, T // 2, T - 1}):
        x_t = c["x_trj"][t] + 0.01 * rng.normal(size=n)
        lo = np.where(np.isfinite(c["lo"][t:]), c["lo"][t:], np.minimum(c["hi"][t:], 0.0) - 0.1)
        hi = np.where(np.isfinite(c["hi"][t:]), c["hi"][t:], np.maximum(lo, 0.0) + 0.1)
        z = lo + rng.uniform(size=lo.shape) * (hi - lo)
        q = cc.condensed(c, kind, t, x_t, c["lo"], c["hi"])
        assert (z.reshape(-1) >= q["lo"]).all() and (z.reshape(-1) <= q["hi"]).all()
        s = np.concatenate([x_t, x_t[c["idx"]]])
        cost = 0.0
        for k in range(T - t):
            e = s - prob["sd"][t + k]
            cost += e @ prob["Qs"] @ e + z[k] @ prob["Ru"] @ z[k] + 2.0 * s @ prob["Nc"] @ z[k]
            s = prob["A"][t + k] @ s + prob["B"][t + k] @ z[k] + prob["c"][t + k]
        e = s - prob["sd"][T]
        cost += e @ prob["Qsd"] @ e
        np.testing.assert_allclose(cc.condensed_cost(q, z.reshape(-1)), cost, rtol=1e-12)


def test_mutated_rows_are_what_they_say():
    c = cc.case("hand-abs-gaps-T11")
    lo, hi = cc.mutated_rows(c, "shift")
    assert np.array_equal(lo[:-1], c["lo"][1:]) and np.array_equal(lo[-1], c["lo"][-1])
    assert np.array_equal(hi[:-1], c["hi"][1:])
    lo, hi = cc.mutated_rows(c, "row0")
    assert (lo == c["lo"][0]).all() and (hi == c["hi"][0]).all()
    lo, hi = cc.mutated_rows(c, "swapcol")
    assert np.array_equal(lo[:, ::-1], c["lo"]) and np.array_equal(hi[:, ::-1], c["hi"])
    assert cc.mutated_rows(cc.case("bob-abs-ragged-T11"), "swapcol") is None
    assert cc.mutated_rows(cc.case("hand-abs-ragged-T1"), "shift") is None
    assert cc.mutated_rows(cc.case("hand-abs-ragged-T1"), "row0") is None
