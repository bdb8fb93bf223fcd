"""Admission of the bounded TV-LQR cases (oracle/boxqp_cases.py) that tests/test_boxqp_cases_gpu.py runs on the ADMM
kernel, and the host check of solve_tvlqr's bound arrays.  No GPU.

A case is admitted when
  * the oracle's ADMM converges on it before 40000 iterations at eps 1e-10, at the rho the table records (which is
    the one of 1, 10, 100 with the fewest iterations);
  * the oracle's solution passes the solver-independent KKT certificate at 1e-7: the device is held to 1e-5, the
    reference sits a factor 100 inside that;
  * what it is built for happens: of every kind of bound it declares at least one entry is active within 1e-7; every
    bounded component with more than one finite row keeps a finite row that is NOT active (a component of the
    single-row shapes has one finite row, which binds: there the rows the mask has to leave alone are the
    infinite ones); and the solution is more than 1e-2 from the unconstrained one;
  * it can see the errors it exists for: the oracle re-solved with the bound rows shifted by one step (either way),
    with lo and hi swapped in sign, and with row 0 used at every step lands more than 1e-4 from the true
    solution -- 1000 x the 1e-7 the device test allows.  Where a mutated solve does not converge, the mutated u and
    du rows must be proved to admit no u sequence (boxqp_cases.u_rows_infeasible, an exact interval recursion): a
    kernel with that error reports failure.  Printed as inf.  A mutation applies to a case when it changes
    an entry the case declares to bind (T = 1 has a single u row: nothing to shift).

Every compiled size keeps at least one case per mutation.
"""
import numpy as np
import pytest

from oracle import boxqp_cases as bc

MUTATIONS = ("shift+", "shift-", "swap", "row0")


@pytest.mark.parametrize("cid", list(bc.CASES))
def test_case_is_admitted(cid):
    c = bc.case(cid)
    T, n, m = c["T"], c["At"].shape[1], c["Bt"].shape[2]
    assert (n, m, c["idx"]) == bc.SIZES[c["size"]]
    for k in bc.ROW_KEYS:
        assert c[k].shape == ((T + 1, n) if k[0] == "x" else (T, m)), k
    if c["idx"] is None:
        assert not np.isfinite(c["du_lo"]).any() and not np.isfinite(c["du_hi"]).any()
    # rho: the recorded one is the fastest of the three
    best, its = bc.pick_rho(c)
    assert its[c["rho"]] == its[best], (c["rho"], its)
    # convergence and certificate
    x, u, it = bc.reference(cid)
    assert it == its[c["rho"]] and it < 40000, it
    res = bc.kkt(c, x, u)
    assert max(res) <= 1e-7, res
    # the features
    act, fin = bc.active(c, x, u)
    for group in c["declared"]:
        assert any(act[k][t, j] for k, t, j in group), ("declared bound not active", group[0])
    for k in bc.ROW_KEYS:
        for j in range(c[k].shape[1]):
            if fin[k][:, j].sum() > 1:
                assert (fin[k][:, j] & ~act[k][:, j]).any(), ("every finite row active", k, j)
    d_unc = max(np.abs(x - c["xs"]).max(), np.abs(u - c["us"]).max())
    assert d_unc > 1e-2, d_unc
    # the errors it has to see
    dist = {}
    for name, rows in bc.mutated_rows(c).items():
        xm, um, itm = bc.solve(c, rows=rows, max_iter=10000, eps=1e-8)
        dist[name] = max(np.abs(xm - x).max(), np.abs(um - u).max())
        if itm == 10000:
            # not converged: counted only where the mutated rows are PROVED to admit no u sequence at all
            assert bc.u_rows_infeasible(c, rows), ("mutated solve did not converge, and is not shown infeasible", name)
            dist[name] = np.inf
    print("%-8s rho %5.0f  it %5d  KKT %.1e %.1e %.1e %.1e  active %s  |sol - unconstrained| %.2e  mutations %s" % (
        cid, c["rho"], it, *res, " ".join("%s %d/%d" % (k, act[k].sum(), fin[k].sum()) for k in bc.ROW_KEYS if fin[k].any()),
        d_unc, " ".join("%s %.1e" % (k, dist[k]) if k in dist else "%s n/a" % k for k in MUTATIONS)))
    for name, d in dist.items():
        assert d > 1e-4, (name, d)


def test_every_size_runs_its_shapes_and_keeps_a_case_per_mutation():
    ran = {size: {shape for s, shape, _ in bc.CASES.values() if s == size} for size in bc.SIZES}
    for size, (n, m, idx) in bc.SIZES.items():
        want = {"B2"} if size not in bc.NEW_SIZES else {"B1", "B2", "B3"}
        if idx is not None:
            want.add("B4")
        if size in ("p21", "d21"):
            want |= {"B5", "B5u", "B5x"}
        assert ran[size] == want, (size, ran[size])
        for name in MUTATIONS:
            assert any(name in bc.mutated_rows(bc.case(cid)) for cid, v in bc.CASES.items() if v[0] == size), (size, name)
    assert {T for _, _, T in bc.CASES.values()} == {1, 2, 12}


def test_b2_is_intermittent_and_b4_irregular():
    """What the shapes promise about their rows, read off the rows."""
    for cid, (size, shape, T) in bc.CASES.items():
        c = bc.case(cid)
        m = c["Bt"].shape[2]
        if shape == "B2":
            assert np.isfinite(c["u_lo"][::2, m - 1]).all() and not np.isfinite(c["u_lo"][1::2, m - 1]).any()
            i = int(np.where(np.isfinite(c["x_lo"]).any(axis=0))[0][0])
            assert not np.isfinite(c["x_lo"][:T // 2]).any() and np.isfinite(c["x_hi"][T // 2:, i]).all()
            assert abs(abs(c["x_lo"][T, i]) - abs(c["x_hi"][T, i])) > 1e-3
            assert len(np.unique(c["u_hi"][:, 0])) == T
        if shape == "B4":
            w = c["u_hi"][:, 0] - c["u_lo"][:, 0]
            np.testing.assert_allclose(w, w[0], rtol=1e-12)                       # one width,
            assert len(np.unique(np.round(np.diff(c["u_lo"][:, 0]), 12))) == T - 1    # another offset at every step
            assert not np.isfinite(c["du_lo"][:, 0]).any() and np.isfinite(c["du_hi"]).all()
            assert len(np.unique(c["du_hi"])) == c["du_hi"].size
            if m > 1:
                assert not np.isfinite(c["u_lo"][:, m - 1]).any() and not np.isfinite(c["u_hi"][:, m - 1]).any()
                assert np.isfinite(c["du_lo"][:, 1:]).all()


# ------------------------------------------------------------------------------------------------ the host check
def _call(amd_tv, c, **bounds):
    return amd_tv.solve_tvlqr(c["At"], c["Bt"], c["ct"], c["Q"], c["Qd"], c["R"], c["x0"], c["xd"], None,
                              indices_u_into_x=c["idx"], **bounds)


@pytest.mark.parametrize("cid", ["p62-B2", "d52-B2"])
def test_solve_tvlqr_refuses_bound_arrays_of_the_wrong_shape(cid, monkeypatch):
    """A bound array is (2, width) or (2, rows, width) with rows = T + 1 for x_bound_abs and T for u_bound_abs /
    u_bound_rel: the kernel reads exactly that many rows.  Anything else is a ValueError that names the argument and
    the shape, raised before a tensor goes to the device (here: to_dev must not be reached)."""
    from irs_mpc_amd import device as dev
    from irs_mpc_amd import tv_lqr

    def no_device(*a, **k):
        raise AssertionError("a tensor was moved to the device before the bound arrays were checked")

    monkeypatch.setattr(dev, "to_dev", no_device)
    c = bc.case(cid)
    T, n, m = c["T"], c["At"].shape[1], c["Bt"].shape[2]
    two = lambda rows, width: np.stack([np.full((rows, width), -1.0), np.full((rows, width), 1.0)])
    bad = [("x_bound_abs", two(T, n), (T + 1, n)), ("x_bound_abs", two(T + 2, n), (T + 1, n)),
           ("u_bound_abs", two(T - 1, m), (T, m)), ("u_bound_abs", two(T + 1, m), (T, m)),
           ("x_bound_abs", two(T + 1, n + 1), (T + 1, n)), ("u_bound_abs", two(T, m + 1), (T, m)),
           ("u_bound_abs", np.ones((2, m + 1)), (T, m)), ("x_bound_abs", np.ones((3, n)), (T + 1, n)),
           ("u_bound_rel", two(T - 1, m), (T, m)), ("u_bound_rel", two(T, m + 1), (T, m))]
    for name, arr, (rows, width) in bad:
        with pytest.raises(ValueError) as e:
            _call(tv_lqr, c, **{name: arr})
        msg = str(e.value)
        assert name in msg and str(arr.shape) in msg, msg
        assert "(2, %d)" % width in msg and "(2, %d, %d)" % (rows, width) in msg, msg
    # well-formed arrays pass the check: the next thing the call does is move data to the device
    for name, arr in (("x_bound_abs", two(T + 1, n)), ("x_bound_abs", np.ones((2, n))), ("u_bound_abs", two(T, m)),
                      ("u_bound_abs", np.ones((2, m))), ("u_bound_rel", two(T, m))):
        with pytest.raises(AssertionError, match="moved to the device"):
            _call(tv_lqr, c, **{name: arr})
