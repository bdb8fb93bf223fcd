"""The cases of oracle/plan_cases.py, admitted here without a GPU: every case says what it claims to say on the
statement itself, the placement rule sends the cases to the kernels they are meant for, rounding cannot move a
generic case's flag, every way to get the plan test wrong in the list below changes the flag of an admitted case,
and the project's host statement (IrsLqr._tail_plans_within_bounds) agrees with the statement on every case."""
import types

import numpy as np
import pytest

from oracle import plan_cases as pc

SHAPE_IDS = ["%d-%d-%d" % key for key in pc.SHAPES]


def all_cases(family=None, max_T=None):
    for (n, m, T) in pc.SHAPES:
        if max_T is not None and T > max_T:
            continue
        for fam in pc.FAMILIES if family is None else (family,):
            yield from pc.cases(n, m, T, fam)


# ------------------------------------------------------------------------------------------------ admission
@pytest.mark.parametrize("key", list(pc.SHAPES), ids=SHAPE_IDS)
def test_every_case_is_admitted_and_every_required_one_is_there(key):
    n, m, T = key
    for fam in pc.FAMILIES:
        cs = pc.cases(n, m, T, fam)
        for c in cs:
            plan = pc.case_plan(c)
            assert pc.admit(c, plan) is None, (pc.describe(c), pc.admit(c, plan))
            assert pc.within(plan, *c["bounds"]) == (c["want"] == 0), pc.describe(c)
        shapes = [c["shape"] for c in cs]
        full = "touch" if fam == "exact" else "snug"
        assert shapes.count(full) == 1 and shapes.count("open") == 1 and shapes.count("open-mixed") == 1
        inward = {(c["target"]["kind"], c["target"]["side"], c["target"]["comp"]) for c in cs if c["shape"] == full + "-in"}
        if fam == "exact":
            assert inward == {(kind, side, i) for kind, w in (("x", n), ("u", m)) for side in ("lo", "hi")
                              for i in (0, w - 1)}
        tails = {c["target"]["t"] for c in cs if c["shape"] == "one-tail"}
        assert tails == set(pc.required_tails(n, m, T)), (tails, pc.required_tails(n, m, T))
        # the first control of the last tail alone
        assert any(c["shape"] == "one-tail" and c["target"]["t"] == T - 1 and c["target"]["kind"] == "u" for c in cs)
        steps = {(c["target"]["s"], c["target"]["via"], c["target"]["kind"]) for c in cs if c["shape"] == "one-step"}
        assert {(T - 1, "k", "u"), (T - 1, "ct", "x")} <= steps and any(s == 0 for s, _, _ in steps), steps
        # exactly one bound is finite in the one-tail and one-step cases, and the moved array alone differs
        for c in cs:
            if c["shape"] in ("one-tail", "one-step"):
                assert sum(int(np.isfinite(b).sum()) for b in c["bounds"]) == 1
                (name, arr), = c["override"].items()
                diff = np.argwhere(arr != pc.problem(n, m, T, fam)[name])
                row = c["target"]["t"] if name == "x_new" else c["target"]["s"]
                assert len(diff) == 1 and diff[0][0] == row, pc.describe(c)
                if fam == "exact":
                    assert float(arr[tuple(diff[0])]).is_integer()


def test_generic_family_has_inward_cases_of_every_kind_and_side():
    seen = {(c["target"]["kind"], c["target"]["side"], "first" if c["target"]["comp"] == 0 else "last")
            for c in all_cases("generic") if c["shape"] == "snug-in"}
    assert len(seen) == 8, seen


def test_recorded_seeds_are_the_first_that_admit():
    for (n, m, T, fam), seed in pc.SEED.items():
        assert seed > 0 and (n, m, T) in pc.SHAPES
        assert pc.find_seed(n, m, T, fam) == seed


def test_touching_is_inside_and_infinity_never_binds():
    """The semantics on three numbers: strict compare; a value equal to its bound is inside; +-inf never binds."""
    U = np.array([[[1.0]]], dtype=pc.LD)
    X = np.array([[[np.nan], [2.0]]], dtype=pc.LD)
    inf = np.inf
    assert pc.within((U, X), [2.0], [2.0], [1.0], [1.0])
    assert pc.within((U, X), [-inf], [inf], [-inf], [inf])
    assert not pc.within((U, X), [-inf], [np.nextafter(2.0, 0.0)], [-inf], [inf])
    assert not pc.within((U, X), [-inf], [inf], [np.nextafter(1.0, 2.0)], [inf])
    # a longdouble value one longdouble ulp beyond an f64 bound is beyond
    assert not pc.within((U + np.finfo(pc.LD).eps, X), [-inf], [inf], [-inf], [1.0])


# ------------------------------------------------------------------------------------------------ placement
def test_placement_reaches_both_kernels_on_every_size():
    for (n, m, T), meant in pc.SHAPES.items():
        assert pc.placement(n, m, T) == meant, (n, m, T)
        assert all(c["placement"] == meant for fam in pc.FAMILIES for c in pc.cases(n, m, T, fam))
    fast = [key for key, meant in pc.SHAPES.items() if meant == "fast"]
    assert len(fast) >= 20 and {n for n, _, _ in fast} == set(range(1, 17))
    assert {(n, m) for n, m, _ in fast} >= {(1, 2), (3, 16), (16, 16)}                  # m > n, m = 16, n = m = 16
    assert {T for n, m, T in fast if (n, m) in ((2, 1), (3, 2))} >= set(pc.EDGE_T)
    assert {"serial-n", "serial-lds", "serial-multipass"} <= set(pc.SHAPES.values())
    # the rule at its edge: n = m = 16 fits LDS at T = 35 and not at 36; one byte of state more and it is the serial one
    assert pc.placement(16, 16, 35) == "fast" and pc.placement(16, 16, 36) == "serial-lds"
    assert pc.placement(17, 1, 1) == "serial-n" and pc.placement(2, 1, 300) == "fast"
    assert pc.pass_size(12, 4, 300) == 256 and pc.pass_size(2, 1, 200) == 64 and pc.pass_size(2, 1, 5) == 8


# ------------------------------------------------------------------------------------------------ rounding
def walk64(d, start=None, first=None, kshift=0, use_c=True, use_k=True, closed_loop=False):
    """The plan in f64, (U, X) as pc.plans lays them out.  Defaults: the statement, u then x.  closed_loop: x+ = (A + B
    K) x + (B k + c).  The other arguments are the mutants' (below): tail t takes x_new[start[t]], walks from step
    first[t], reads K and k of step s + kshift, and leaves c or k out."""
    A, B, c, K, k, x_new = (np.asarray(d[key], dtype=float) for key in pc.DATA_KEYS)
    T, n, m = B.shape
    ts = np.arange(T)
    start = ts if start is None else start
    first = ts if first is None else first
    U, X = np.full((T, T, m), np.nan), np.full((T, T + 1, n), np.nan)
    x = np.zeros((T, n))
    for s in range(T):
        x[first == s] = x_new[start[first == s]]
        on = first <= s
        sk = min(s + kshift, T - 1)
        ks = k[sk] if use_k else 0.0
        cs = c[s] if use_c else 0.0
        u = x[on] @ K[sk].T + ks
        if closed_loop:
            x[on] = x[on] @ (A[s] + B[s] @ K[sk]).T + (B[s] @ (k[sk] if use_k else np.zeros(m)) + cs)
        else:
            x[on] = x[on] @ A[s].T + u @ B[s].T + cs
        U[on, s], X[on, s + 1] = u, x[on]
    return U, X


@pytest.mark.parametrize("key", list(pc.SHAPES), ids=SHAPE_IDS)
def test_generic_family_rounding_is_far_inside_the_margin(key):
    """The f64 plan, u then x and in the closed-loop form, differs from the longdouble plan by less than 1e-3 of the
    case's margin, per component: the flag of a generic case does not depend on how a kernel rounds."""
    n, m, T = key
    worst = 0.0
    for c in pc.cases(n, m, T, "generic"):
        ok, Uv, Xv = pc.entries(pc.case_plan(c))
        for closed_loop in (False, True):
            U64, X64 = walk64(pc.case_data(c), closed_loop=closed_loop)
            eu = np.abs(U64[ok] - Uv).max(axis=0) / c["margin"]["u"]
            ex = np.abs(X64[:, 1:][ok] - Xv).max(axis=0) / c["margin"]["x"]
            worst = max(worst, float(eu.max()), float(ex.max()))
            assert eu.max() < 1e-3 and ex.max() < 1e-3, (pc.describe(c), closed_loop, float(eu.max()), float(ex.max()))
    print("%s: worst f64 error / margin %.3g" % (key, worst))


# ------------------------------------------------------------------------------------------------ mutants
def _flag(Uv, Xv, bounds, strict=True, f32=False):
    xlo, xhi, ulo, uhi = bounds
    if f32:
        Uv, Xv = Uv.astype(np.float32), Xv.astype(np.float32)
        xlo, xhi, ulo, uhi = (np.asarray(b, dtype=np.float32) for b in bounds)
    if strict:
        out = (Uv < ulo).any() or (Uv > uhi).any() or (Xv < xlo).any() or (Xv > xhi).any()
    else:
        out = (Uv <= ulo).any() or (Uv >= uhi).any() or (Xv <= xlo).any() or (Xv >= xhi).any()
    return int(out)


def mutant_flag(name, c, plan):
    """The flag a wrong plan test would give on case c: the list of the issue, as variants of within / plans."""
    n, m, T = c["n"], c["m"], c["T"]
    xlo, xhi, ulo, uhi = (np.array(b, dtype=float) for b in c["bounds"])
    ts = np.arange(T)
    walks = {
        "starts tail t from x_new[t-1]": dict(start=np.maximum(ts - 1, 0)),
        "starts tail t from x_new[t+1]": dict(start=ts + 1),
        "adopts the state from the wave's earliest tail": dict(first=ts // 4 * 4),
        "uses K_{s+1} at step s": dict(kshift=1),
        "omits c": dict(use_c=False),
        "omits k": dict(use_k=False),
    }
    if name in walks:
        plan = walk64(pc.case_data(c), **walks[name])
    ok, Uv, Xv = pc.entries(plan)
    tt, ss = np.nonzero(ok)
    keep_u = keep_x = np.ones(len(tt), dtype=bool)
    kw = {}
    if name == "skips tail T-1":
        keep_u = keep_x = tt != T - 1
    elif name == "skips tail 0":
        keep_u = keep_x = tt != 0
    elif name == "skips the tails t = 63 (mod 64)":
        keep_u = keep_x = tt % 64 != 63
    elif name == "skips every tail past the first 64":
        keep_u = keep_x = tt < 64
    elif name == "ignores u bounds":
        ulo[:], uhi[:] = -np.inf, np.inf
    elif name == "ignores x bounds":
        xlo[:], xhi[:] = -np.inf, np.inf
    elif name == "ignores lower sides":
        xlo[:], ulo[:] = -np.inf, -np.inf
    elif name == "ignores upper sides":
        xhi[:], uhi[:] = np.inf, np.inf
    elif name == "checks only components < min(n, m)":
        q = min(n, m)
        xlo[q:], xhi[q:], ulo[q:], uhi[q:] = -np.inf, np.inf, -np.inf, np.inf
    elif name == "drops component n-1":
        xlo[n - 1], xhi[n - 1] = -np.inf, np.inf
    elif name == "drops component m-1":
        ulo[m - 1], uhi[m - 1] = -np.inf, np.inf
    elif name == "reads u bounds with x's component index":       # lane i reads bound [i < n ? i : 0] for both
        idx = np.where(np.arange(m) < n, np.arange(m), 0)
        ulo, uhi = ulo[idx], uhi[idx]
    elif name == "omits X[T]":
        keep_x = ss != T - 1
    elif name == "omits the first control of each tail":
        keep_u = ss != tt
    elif name == "non-strict compare":
        kw = dict(strict=False)
    elif name == "compares after rounding to f32":
        kw = dict(f32=True)
    else:
        assert name in walks, name
    return _flag(Uv[keep_u], Xv[keep_x], (xlo, xhi, ulo, uhi), **kw)


MUTANTS = ["skips tail T-1", "skips tail 0", "skips the tails t = 63 (mod 64)", "skips every tail past the first 64",
           "starts tail t from x_new[t-1]", "starts tail t from x_new[t+1]",
           "adopts the state from the wave's earliest tail", "ignores u bounds", "ignores x bounds",
           "ignores lower sides", "ignores upper sides", "checks only components < min(n, m)", "drops component n-1",
           "drops component m-1", "reads u bounds with x's component index", "omits X[T]",
           "omits the first control of each tail", "uses K_{s+1} at step s", "omits c", "omits k",
           "non-strict compare", "compares after rounding to f32"]
PRECISION = ("non-strict compare", "compares after rounding to f32")


def test_every_mutant_is_caught_in_each_family():
    """Every mutant gives the wrong flag on an admitted case of each family (the two precision mutants: of the exact
    family), on the shapes up to T = 65 alone.  Prints which cases catch which mutant."""
    caught = {(name, fam): [] for name in MUTANTS for fam in pc.FAMILIES}
    for c in all_cases(max_T=65):
        plan = pc.case_plan(c)
        assert _flag(*pc.entries(plan)[1:], c["bounds"]) == c["want"]           # the unmutated restatement
        for name in MUTANTS:
            if mutant_flag(name, c, plan) != c["want"]:
                caught[name, c["family"]].append(c["id"])
    missing = []
    for name in MUTANTS:
        for fam in pc.FAMILIES:
            ids = caught[name, fam]
            print("%-48s %-8s %4d cases, e.g. %s" % (name, fam, len(ids), ", ".join(ids[:3])))
            if not ids and not (fam == "generic" and name in PRECISION):
                missing.append((name, fam))
    assert not missing, missing


# ------------------------------------------------------------------------------------------------ the host statement
@pytest.mark.parametrize("key", list(pc.SHAPES), ids=SHAPE_IDS)
def test_host_statement_gives_the_statements_answer(key):
    """IrsLqr._tail_plans_within_bounds, on a stand-in that carries what the method reads, with CPU tensors."""
    import torch
    from irs_mpc_amd.irs_lqr import IrsLqr
    n, m, T = key
    for fam in pc.FAMILIES:
        for c in pc.cases(n, m, T, fam):
            d = pc.case_data(c)
            sol = types.SimpleNamespace(_box_host=tuple(c["bounds"]), T=T, dim_x=n)
            got = IrsLqr._tail_plans_within_bounds(sol, *[torch.from_numpy(np.array(d[k])) for k in pc.DATA_KEYS])
            assert bool(got) == (c["want"] == 0), pc.describe(c)
