"""Every bounded-ADMM entry of the C ABI (csrc/boxqp_api.hip) delivers its pointers to the right fields: the entries
that no other GPU test calls -- irs_tvlqr_box_descent, _if, irs_tvlqr_box_solve, irs_quasistatic_box_descent, _ws --
called through ctypes beside their _wsx / _set siblings, which run the same kernel on the same arguments.  The
results are equal bit for bit, and one entry of each family is held to the oracle at the tolerance of the
neighbouring tests of that entry (tests/test_boxqp_cases_gpu.py, tests/test_gpu_parity.py).

Two problems, the smallest there are, T = 4: the pendulum (2, 1) with an input box [-0.3, 0.5] that binds, and box on
box (2, 1), the smallest position-controlled model, with a trust region [-0.02, +0.05] around the nominal command and
a rate limit [-0.01, +0.03].  Every box is asymmetric: lo and hi exchanged, or the u and du pairs exchanged, is
another QP with another answer."""
import functools

import numpy as np
import pytest
import torch

from oracle import boxqp_cases as bc
from oracle import ctrlbox_cases as cc
from oracle import irs_oracle as orc

pytestmark = pytest.mark.gpu

T = 4
RELAX, MAX_ITER, EPS = 1.6, 40000, 1e-10
SENTINEL = -777.0


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()     # fails loudly if the HIP library is missing
    return irs_mpc_amd


# ------------------------------------------------------------------------------------------------ the two problems
@functools.lru_cache(maxsize=None)
def pendulum():
    """Swing-up from rest, linearised along a nominal roll-out; constant boxes, one row each (the descent entries'
    form).  The velocity box is never met; the input box binds."""
    so = orc.PendulumOracle(0.05)
    x0, u_trj = np.zeros(2), np.full((T, 1), 0.1)
    x_trj = orc.rollout(so, x0, u_trj)
    At, Bt, ct = orc.exact_TV(so, x_trj, u_trj)
    return dict(sys=so, At=At, Bt=Bt, ct=ct, Q=np.eye(2), Qd=20.0 * np.eye(2), R=np.eye(1),
                xd=np.tile(np.array([np.pi, 0.0]), (T + 1, 1)), x0=x0, idx=None, rho=10.0,
                xlo=np.array([-np.inf, -3.0]), xhi=np.array([np.inf, 4.0]), ulo=np.array([-0.3]), uhi=np.array([0.5]))


@functools.lru_cache(maxsize=None)
def box_on_box():
    """oracle/ctrlbox_cases.py's box-on-box problem at T = 4 with both control boxes as per-time rows."""
    p = dict(cc.problem("bob", T))
    rows = orc.quasistatic_bounds(p["x_trj"], p["idx"], None, np.array([[-0.02], [0.05]]), np.array([[-0.01], [0.03]]))
    p.update(sys=cc.system("bob"), rho=10.0, rows=dict(zip(bc.ROW_KEYS, rows)))
    return p


def rows_tiled(p):
    """The pendulum's constant boxes as the per-time rows the solve entries take."""
    return dict(x_lo=np.tile(p["xlo"], (T + 1, 1)), x_hi=np.tile(p["xhi"], (T + 1, 1)), u_lo=np.tile(p["ulo"], (T, 1)),
                u_hi=np.tile(p["uhi"], (T, 1)), du_lo=np.full((T, 1), -np.inf), du_hi=np.full((T, 1), np.inf))


# ------------------------------------------------------------------------------------------------ the calls
class Call:
    """The device side of one problem: its arrays on the GPU, fresh outputs per call, the results as numpy."""

    def __init__(self, dm, p, n, m):
        from irs_mpc_amd import _lib, device as dev
        self.lib, self._lib, self.dev, self.dm, self.n, self.m = _lib.load(), _lib, dev, dm, n, m
        self.head = [dm.model_id, dm._p, dm._np, T]
        self.d = {k: dev.to_dev(p[k]) for k in ("At", "Bt", "ct", "Q", "Qd", "R", "xd", "x0")}
        self.rho = p["rho"]

    def ptrs(self, *names):
        return [self.d[k].data_ptr() for k in names]

    def rows(self, rows, keys):
        """Device pointers of bound rows (kept alive on self); a row without a finite entry is a null pointer."""
        self.keep = [self.dev.to_dev(rows[k]) if np.isfinite(rows[k]).any() else None for k in keys]
        return [t.data_ptr() if t is not None else None for t in self.keep]

    def scalars(self):
        return [self.rho, RELAX, MAX_ITER, EPS]

    def settings(self):
        self.st = self._lib.admm_settings(self.rho, RELAX, MAX_ITER, EPS, adaptive=False)
        return self.st

    def outputs(self, cost):
        o = dict(x=torch.full((T + 1, self.n), SENTINEL, dtype=self.dev.F64, device="cuda"),
                 u=torch.full((T, self.m), SENTINEL, dtype=self.dev.F64, device="cuda"),
                 info=torch.full((3,), -7, dtype=torch.int32, device="cuda"))
        if cost:
            o["cost"] = torch.full((1,), SENTINEL, dtype=self.dev.F64, device="cuda")
        return o

    def run(self, entry, args, o):
        self._lib.check(getattr(self.lib, entry)(*self.head, *args, self.dev._stream()), entry)
        return {k: v.cpu().numpy() for k, v in o.items()}


def assert_same(results, keys=("x", "u", "info")):
    first = next(iter(results))
    for name, r in results.items():
        for k in keys:
            np.testing.assert_array_equal(r[k], results[first][k], err_msg="%s of %s vs %s" % (k, name, first))


def report(what, got, want, **tol):
    """Print the figure, then assert it."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    print("%s: max abs err %.3g" % (what, np.abs(got - want).max()))
    np.testing.assert_allclose(got, want, err_msg=what, **tol)


# ------------------------------------------------------------------------------------------------ the descent entries
def descent_prefix(c, p):
    """The arguments the descent entries share, from At to the four constant bound rows (kept alive on c)."""
    c.bounds = [c.dev.to_dev(p[k]) for k in ("xlo", "xhi", "ulo", "uhi")]
    return [*c.ptrs("At", "Bt", "ct", "Q", "Qd", "R"), 0.5, *c.ptrs("xd", "x0"), *[t.data_ptr() for t in c.bounds]]


def test_descent_entries_agree_and_match_the_oracle(amd):
    """irs_tvlqr_box_descent == _if (null run_flag) == _wsx (null workspace) == _set (adaptive = 0), and the oracle's
    local_descent_box at the tolerances of test_box_descent_vs_oracle / test_three_cart_box_descent_vs_oracle."""
    p = pendulum()
    c = Call(amd.PendulumDynamics(0.05).dm(), p, 2, 1)
    pre = descent_prefix(c, p)
    res = {}
    o = c.outputs(False)
    res["descent"] = c.run("irs_tvlqr_box_descent", pre + c.scalars() + [o["x"].data_ptr(), o["u"].data_ptr(),
                                                                         o["info"].data_ptr()], o)
    o = c.outputs(True)
    res["if"] = c.run("irs_tvlqr_box_descent_if", pre + c.scalars() + [
        o["x"].data_ptr(), o["u"].data_ptr(), o["cost"].data_ptr(), o["info"].data_ptr(), None], o)
    o = c.outputs(False)
    res["wsx"] = c.run("irs_tvlqr_box_descent_wsx", pre + c.scalars() + [
        o["x"].data_ptr(), o["u"].data_ptr(), o["info"].data_ptr(), None, 0], o)
    o = c.outputs(False)
    res["set"] = c.run("irs_tvlqr_box_descent_set", pre + [c.settings(), o["x"].data_ptr(), o["u"].data_ptr(),
                                                           o["info"].data_ptr(), None, None, 0], o)
    assert_same(res)
    r = res["if"]
    assert r["info"][0] == 0 and r["info"][2] == 0, r["info"]
    xo, uo, iters = orc.local_descent_box(p["sys"], p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["x0"],
                                          p["xd"], p["xlo"], p["xhi"], p["ulo"], p["uhi"], rho=p["rho"],
                                          max_iter=MAX_ITER, eps=EPS)
    assert max(iters) < MAX_ITER, iters
    report("u_new vs oracle", r["u"], uo, rtol=1e-5, atol=1e-6)
    report("x_new vs oracle", r["x"], xo, rtol=1e-5, atol=1e-6)
    assert r["u"].max() == pytest.approx(0.5, abs=1e-9) and r["u"].min() > -0.3        # the upper side binds


def test_descent_if_returns_at_once_on_a_zero_flag(amd):
    """irs_tvlqr_box_descent_if with *run_flag == 0: nothing is written; with 1: the descent of the other entries."""
    p = pendulum()
    c = Call(amd.PendulumDynamics(0.05).dm(), p, 2, 1)
    pre = descent_prefix(c, p)
    res = {}
    for flag in (0, 1, None):
        f = None if flag is None else torch.full((1,), flag, dtype=torch.int32, device="cuda")
        o = c.outputs(True)
        res[flag] = c.run("irs_tvlqr_box_descent_if", pre + c.scalars() + [
            o["x"].data_ptr(), o["u"].data_ptr(), o["cost"].data_ptr(), o["info"].data_ptr(),
            None if f is None else f.data_ptr()], o)
    for k in ("x", "u", "cost"):
        assert (res[0][k] == SENTINEL).all(), k
    assert (res[0]["info"] == -7).all()
    assert_same({1: res[1], None: res[None]}, ("x", "u", "info", "cost"))
    assert (res[1]["u"] != SENTINEL).all() and res[1]["info"][0] == 0


# ------------------------------------------------------------------------------------------------ the solve entries
@pytest.mark.parametrize("which", ["pendulum", "box_on_box"])
def test_solve_entries_agree_and_match_the_oracle(amd, which):
    """irs_tvlqr_box_solve == _wsx (null workspace) == _set (adaptive = 0) on the plain and on the position-controlled
    form, and the oracle's ADMM on the same QP at atol 1e-7 (test_case_kkt_certified_and_equal_to_the_oracle)."""
    if which == "pendulum":
        p, dm, du = pendulum(), amd.PendulumDynamics(0.05).dm(), False
        rows = rows_tiled(p)
    else:
        p, dm, du = box_on_box(), amd.BoxOnBoxDynamics(0.1, 1.0, 100.0).dm(), True
        rows = p["rows"]
    c = Call(dm, p, 2, 1)
    alpha = 1.0 if du else 0.5
    pre = [*c.ptrs("At", "Bt", "ct", "Q", "Qd", "R"), alpha, *c.ptrs("xd", "x0"), 1 if du else 0,
           *c.rows(rows, bc.ROW_KEYS)]
    res = {}
    o = c.outputs(False)
    res["solve"] = c.run("irs_tvlqr_box_solve", pre + c.scalars() + [o["x"].data_ptr(), o["u"].data_ptr(),
                                                                     o["info"].data_ptr()], o)
    o = c.outputs(False)
    res["wsx"] = c.run("irs_tvlqr_box_solve_wsx", pre + c.scalars() + [o["x"].data_ptr(), o["u"].data_ptr(),
                                                                       o["info"].data_ptr(), None, 0], o)
    o = c.outputs(False)
    res["set"] = c.run("irs_tvlqr_box_solve_set", pre + [c.settings(), o["x"].data_ptr(), o["u"].data_ptr(),
                                                         o["info"].data_ptr(), None, None, 0], o)
    assert_same(res)
    r = res["solve"]
    assert r["info"][0] == 0 and r["info"][2] == 0, r["info"]
    case = dict(At=p["At"], Bt=p["Bt"], ct=p["ct"], Q=p["Q"], Qd=p["Qd"], R=p["R"], x0=p["x0"], xd=p["xd"],
                idx=p["idx"], rho=p["rho"])
    xo, uo, it = bc.solve(case, rows=rows, max_iter=MAX_ITER, eps=EPS)
    assert it < MAX_ITER
    report("u* vs oracle ADMM", r["u"], uo, rtol=0, atol=1e-7)
    report("x* vs oracle ADMM", r["x"], xo, rtol=0, atol=1e-7)
    binds(r["x"], r["u"], p, rows)


def binds(x, u, p, rows):
    """The plan meets a finite u row and, position controlled, a finite du row -- and no bound is broken."""
    assert (u >= rows["u_lo"] - 1e-7).all() and (u <= rows["u_hi"] + 1e-7).all()
    assert (np.abs(u - rows["u_lo"]) < 1e-7).any() or (np.abs(u - rows["u_hi"]) < 1e-7).any(), "no u bound binds"
    if p["idx"] is not None:
        d = np.diff(np.vstack([p["x0"][list(p["idx"])][None], u]), axis=0)
        assert (d >= rows["du_lo"] - 1e-7).all() and (d <= rows["du_hi"] + 1e-7).all()
        assert (np.abs(d - rows["du_lo"]) < 1e-7).any() or (np.abs(d - rows["du_hi"]) < 1e-7).any(), "no du bound binds"


# ------------------------------------------------------------------------------------------------ the quasistatic entries
def test_quasistatic_entries_agree_and_match_the_oracle(amd):
    """irs_quasistatic_box_descent == _ws == _wsx (null workspace) == _set (adaptive = 0), all with solver 1, and the
    oracle's local_descent_quasistatic at the tolerances of test_box_pivoting_admm_descent_vs_oracle."""
    p = box_on_box()
    rows = p["rows"]
    c = Call(amd.BoxOnBoxDynamics(0.1, 1.0, 100.0).dm(), p, 2, 1)
    pre = [*c.ptrs("At", "Bt", "ct", "Q", "Qd", "R", "xd", "x0"), *c.rows(rows, bc.ROW_KEYS), 1]

    def outs(o):
        return [o["x"].data_ptr(), o["u"].data_ptr(), o["cost"].data_ptr(), o["info"].data_ptr()]
    res = {}
    o = c.outputs(True)
    res["descent"] = c.run("irs_quasistatic_box_descent", pre + c.scalars() + outs(o), o)
    o = c.outputs(True)
    res["ws"] = c.run("irs_quasistatic_box_descent_ws", pre + c.scalars() + outs(o) + [None], o)
    o = c.outputs(True)
    res["wsx"] = c.run("irs_quasistatic_box_descent_wsx", pre + c.scalars() + outs(o) + [None, None, 0], o)
    o = c.outputs(True)
    res["set"] = c.run("irs_quasistatic_box_descent_set", pre + [c.settings()] + outs(o) + [None, None, 0], o)
    assert_same(res, ("x", "u", "info", "cost"))
    r = res["descent"]
    assert r["info"][0] == 0 and r["info"][2] == 0, r["info"]
    xo, uo, iters = orc.local_descent_quasistatic(p["sys"], p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["x0"],
                                                  p["xd"], *[rows[k] for k in bc.ROW_KEYS], rho=p["rho"],
                                                  max_iter=MAX_ITER, eps=EPS, relax=RELAX)
    assert max(iters) < MAX_ITER, iters
    report("u_new vs oracle", r["u"], uo, rtol=0, atol=2e-7)
    report("x_new vs oracle", r["x"], xo, rtol=0, atol=2e-7)
    report("cost", r["cost"][0], orc.eval_cost_quasistatic(xo, uo, p["xd"], p["Q"], p["Qd"], p["R"], p["idx"]), rtol=1e-7)
    # both boxes bind: the trust region around the nominal command, and the rate limit from the realised position
    assert np.isclose((r["u"] - rows["u_hi"]).max(), 0.0, atol=1e-7) or np.isclose((r["u"] - rows["u_lo"]).min(), 0.0,
                                                                                  atol=1e-7)
    d = (r["u"] - r["x"][:-1, p["idx"]])
    assert np.isclose(d.max(), 0.03, atol=1e-7) or np.isclose(d.min(), -0.01, atol=1e-7)
