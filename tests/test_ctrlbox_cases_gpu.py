"""The active-set descent kernels (csrc/ctrlbox.hip: solver 2, lanes; csrc/ctrlbox_mfma.hip: solver 3, tiles, and the
batched entry) on irregular control boxes: the cases of oracle/ctrlbox_cases.py, admitted by
tests/test_ctrlbox_cases_cpu.py.

Every finished descent goes through `certify`, which checks it TAIL BY TAIL: u_new[t] against the certified optimum of
tail t .. T-1 started from the device's own realised x_new[t] (atol 1e-8, the suite's figure for these kernels against
their twin), x_new[t + 1] against the device's own contact step of (x_new[t], u_new[t]) (atol 1e-9) and the cost
against eval_cost (rtol 1e-10) -- the last two are the figures of test_quasistatic_descent_outputs_are_self_consistent.
An error in one tail shows at that tail, and the stiff contact step amplifies nothing.  The reference of a tail is the
ORIGINAL QP condensed to a dense H z + g, with a candidate accepted only on its optimality conditions
(ctrlbox_cases.tail_reference): no restatement of the kernels' algorithm decides what is right.

The cases are built so that a bound row read one step off, row 0 broadcast or the components reversed moves some
first control by more than 1e-4 (the CPU admission holds them to that).
"""
import numpy as np
import pytest
import torch

from oracle import ctrlbox_cases as cc
from oracle import irs_oracle as orc

pytestmark = pytest.mark.gpu

SOLVERS = (2, 3)                       # active set on lanes / on matrix-core tiles
OTHER = {"exact": "pgs", "pgs": "exact"}
MAIN_CONTACT = "exact"                 # the contact solver the full shape list runs on (the default of the models)


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()     # fails loudly if the HIP library is missing
    return irs_mpc_amd


def report(what, got, want, **tol):
    """Print the figure, then assert it."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    err = np.abs(got - want)
    print("%s: max abs err %.3g, worst err / (atol + rtol |want|) %.3g" % (
        what, err.max(), (err / np.maximum(tol.get("atol", 0) + tol["rtol"] * np.abs(want), 1e-300)).max()))
    np.testing.assert_allclose(got, want, err_msg=what, **tol)


_SYSTEMS = {}


def device_system(amd, model, contact=MAIN_CONTACT):
    """The device twin of a case's model (box-on-box has one contact solver)."""
    key = (model, contact if model != "bob" else None)
    if key not in _SYSTEMS:
        _SYSTEMS[key] = {"hand": lambda: amd.PlanarHandDynamics(0.1, contact_solver=contact),
                         "pivot": lambda: amd.BoxPivotingDynamics(0.1, contact_solver=contact),
                         "push": lambda: amd.BoxPushingDynamics(0.1, contact_solver=contact),
                         "bob": lambda: amd.BoxOnBoxDynamics(0.1, 1.0, 100.0)}[model]()
    return _SYSTEMS[key]


def problem_args(c):
    from irs_mpc_amd import device as dev
    return [dev.to_dev(c[k]) for k in ("At", "Bt", "ct", "Q", "Qd", "R", "xd", "x0")]


def row_args(c, lo=None, hi=None):
    """The bound keywords of a case (with other rows in place of its own): none at all for `none`."""
    from irs_mpc_amd import device as dev
    if c["null"] and lo is None:
        return {}
    lo, hi = (c["lo"], c["hi"]) if lo is None else (lo, hi)
    names = ("u_lo", "u_hi") if c["kind"] == "abs" else ("du_lo", "du_hi")
    return {names[0]: dev.to_dev(lo), names[1]: dev.to_dev(hi)}


def to_host(o):
    return {k: o[k].cpu().numpy().copy() for k in ("x_new", "u_new", "cost", "info")}


def descend(dm, c, solver, act=None, lo=None, hi=None):
    """One device descent of the case: dict(x_new, u_new, cost, info) on the host."""
    o = dm.quasistatic_box_descent(*problem_args(c), solver=solver, max_iter=2000, eps=1e-10, act=act,
                                   **row_args(c, lo, hi))
    return to_host(o)


def certify(c, out, dm, what):
    """The tail-by-tail check of a finished device descent `out` of case `c` (module docstring).  Returns the
    certified tails (ctrlbox_cases.certify_trajectory)."""
    from irs_mpc_amd import device as dev
    info = out["info"]
    assert info[0] == 0 and info[2] == 0, (what, info)
    x, u = out["x_new"], out["u_new"]
    np.testing.assert_array_equal(x[0], c["x0"])
    cert = cc.certify_trajectory(c, x, u)
    assert cert["converged"] and cert["ok"], (what, cert["worst"])
    both = c["lo"] == c["hi"]
    n_lo, n_hi = int((cert["at_lo"] & ~both).sum()), int((cert["at_hi"] & ~both).sum())
    print("%s %s: at lo %d, at hi %d of %d; worst certificate residual %.2g" % (c["id"], what, n_lo, n_hi, u.size,
                                                                                 cert["worst"]))
    report("%s %s u_new vs certified tails" % (c["id"], what), u, cert["u"], rtol=0, atol=1e-8)
    step = dm.dynamics_batch(dev.to_dev(x[:-1]), dev.to_dev(u)).cpu().numpy()
    report("%s %s x_new vs the device's own contact step" % (c["id"], what), x[1:], step, rtol=0, atol=1e-9)
    report("%s %s cost %.17g" % (c["id"], what, float(out["cost"].reshape(-1)[0])), float(out["cost"].reshape(-1)[0]),
           orc.eval_cost_quasistatic(x, u, c["xd"], c["Q"], c["Qd"], c["R"], c["idx"]), rtol=1e-10)
    if cc.binds(c):
        assert n_lo + n_hi >= c["m"], (what, "the case stopped binding", n_lo, n_hi)
    else:
        assert n_lo + n_hi == 0
    return cert


# ------------------------------------------------------------------------------------------------ every case
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("cid", list(cc.CASES))
def test_case_is_certified_tail_by_tail(amd, cid, solver):
    c = cc.case(cid)
    dm = device_system(amd, c["model"]).dm()
    assert dm.quasistatic_descent_supported(c["T"], solver), (c["model"], c["T"], solver)
    certify(c, descend(dm, c, solver), dm, "solver %d" % solver)


def test_both_kernels_run_all_four_models_at_these_horizons(amd):
    for model in cc.MODELS:
        dm = device_system(amd, model).dm()
        for T in cc.T_MAIN + cc.T_SHORT:
            for solver in SOLVERS:
                assert dm.quasistatic_descent_supported(T, solver), (model, T, solver)


OTHER_CONTACT = [cid for cid, v in cc.CASES.items()
                 if v[0] != "bob" and v[2] in ("ragged", "gaps") and v[3] in cc.T_MAIN]


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("cid", OTHER_CONTACT)
def test_case_with_the_other_contact_solver(amd, cid, solver):
    """The contact step only moves the realised states the tails start from: the same certificate holds."""
    c = cc.case(cid)
    dm = device_system(amd, c["model"], OTHER[MAIN_CONTACT]).dm()
    assert dm.model_id != device_system(amd, c["model"]).dm().model_id
    certify(c, descend(dm, c, solver), dm, "%s contact, solver %d" % (OTHER[MAIN_CONTACT], solver))


@pytest.mark.parametrize("cid", ["hand-abs-gaps-T12", "pivot-rel-one_sided-T11", "push-abs-pinned-T12",
                                 "bob-rel-offzero-T11"])
def test_auto_solver_picks_an_active_set_kernel(amd, cid):
    """Solver 0 with one irregular control box: certified, and bit for bit the output of one of the two kernels."""
    c = cc.case(cid)
    dm = device_system(amd, c["model"]).dm()
    auto = descend(dm, c, 0)
    certify(c, auto, dm, "solver 0")
    same = [all(np.array_equal(auto[k], o[k]) for k in auto) for o in (descend(dm, c, s) for s in SOLVERS)]
    assert any(same), same


# ------------------------------------------------------------------------------------------------ no bounds
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("model", list(cc.MODELS))
@pytest.mark.parametrize("T", cc.T_MAIN)
def test_infinite_rows_equal_no_rows(amd, model, T, solver):
    """Rows that are infinite throughout == null pointers, bit for bit, and both are the unbounded tail optimum.
    Null pointers have no kind: the kernels run them in the u form, and it is the abs rows that are the same
    program on the same numbers.  Infinite rel rows run the du form of the same QP, other arithmetic: they are held
    to the same certificate, tail by tail."""
    dm = device_system(amd, model).dm()
    none = cc.case(cc.cid_of(model, "abs", "none", T))
    a = descend(dm, none, solver)
    certify(none, a, dm, "solver %d" % solver)
    c = cc.case(cc.cid_of(model, "abs", "allinf", T))
    b = descend(dm, c, solver)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    r = cc.case(cc.cid_of(model, "rel", "allinf", T))
    d = descend(dm, r, solver)
    certify(r, d, dm, "solver %d" % solver)


# ------------------------------------------------------------------------------------------------ warm starts
WARM = [cid for cid, v in cc.CASES.items() if v[2] in ("gaps", "one_sided") and v[3] == 12]


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("cid", WARM)
def test_warm_start_pinned_at_infinite_and_wrong_bounds(amd, cid, solver):
    """A warm start of all +1, then all -1: pinned at bounds that are infinite, and mostly wrong.  The descent is
    certified all the same, and the set it hands back is the sign pattern of the certified first tail on every entry
    whose strict-complementarity margin exceeds 1e-6 (at least half of them: the CPU admission holds these cases to
    that), with nothing pinned at an infinite bound."""
    from irs_mpc_amd import device as dev
    c = cc.case(cid)
    dm = device_system(amd, c["model"]).dm()
    for start in (1.0, -1.0):
        act = dev.to_dev(np.full((c["T"], c["m"]), start))
        cert = certify(c, descend(dm, c, solver, act=act), dm, "solver %d, warm start %+d" % (solver, start))
        got = act.cpu().numpy()
        first = cert["refs"][0]
        sure = first["margins"] > 1e-6
        assert sure.mean() >= 0.5, sure.mean()
        assert np.isin(got, (-1.0, 0.0, 1.0)).all()
        np.testing.assert_array_equal(got[sure], first["side"][sure].astype(float))
        assert not ((got > 0) & ~np.isfinite(c["hi"])).any() and not ((got < 0) & ~np.isfinite(c["lo"])).any()
        assert (got != start).any()


# ------------------------------------------------------------------------------------------------ the batched entry
def batch_descend(dm, cs, **kw):
    """The cases `cs` (one model, kind and horizon) as one launch of B = len(cs) problems; per problem the host dict."""
    from irs_mpc_amd import device as dev
    stack = lambda k: dev.to_dev(np.stack([c[k] for c in cs]))
    names = ("u_lo", "u_hi") if cs[0]["kind"] == "abs" else ("du_lo", "du_hi")
    c0 = cs[0]
    o = dm.quasistatic_box_descent_batch(stack("At"), stack("Bt"), stack("ct"), dev.to_dev(c0["Q"]),
                                         dev.to_dev(c0["Qd"]), dev.to_dev(c0["R"]), stack("xd"), stack("x0"),
                                         max_iter=2000, eps=1e-10,
                                         act=dev.to_dev(np.zeros((len(cs), c0["T"], c0["m"]))),
                                         **{names[0]: stack("lo"), names[1]: stack("hi")}, **kw)
    host = to_host(o)
    return [{k: host[k][b] for k in host} for b in range(len(cs))]


def single_descend(dm, c):
    """The single call the batched entry is compared with (test_quasistatic_batch_gpu.py): solver 3, a zero set."""
    from irs_mpc_amd import device as dev
    return descend(dm, c, 3, act=dev.to_dev(np.zeros((c["T"], c["m"]))))


@pytest.mark.parametrize("kind", cc.KINDS)
@pytest.mark.parametrize("model", list(cc.MODELS))
def test_batch_of_five_different_boxes(amd, model, kind):
    """The five shapes of one (model, kind, T = 11) in one launch, B = 5 problems that differ in their bounds only:
    each certified, each bit for bit its single call (test_descent_batch_equals_single_calls_abs claims bit equality);
    and again with the problems in reverse order."""
    dm = device_system(amd, model).dm()
    cs = [cc.case(cc.cid_of(model, kind, shape, 11)) for shape in cc.BOUNDED]
    singles = [single_descend(dm, c) for c in cs]
    for order in (list(range(5)), list(range(4, -1, -1))):
        outs = batch_descend(dm, [cs[i] for i in order])
        for i, out in zip(order, outs):
            if order[0] == 0:
                certify(cs[i], out, dm, "problem %d of 5" % i)
            for k in out:
                np.testing.assert_array_equal(out[k].reshape(-1), singles[i][k].reshape(-1),
                                              err_msg="%s %s" % (cs[i]["id"], k))


@pytest.mark.parametrize("cid", ["hand-abs-gaps-T12", "pivot-rel-gaps-T11"])
def test_records_in_hbm_equal_on_chip(amd, cid):
    """Solver 3's per-step records forced into a workspace (the batched entry with B = 1 places them there at any
    horizon) == the on-chip single call, bit for bit; certified."""
    c = cc.case(cid)
    dm = device_system(amd, c["model"]).dm()
    assert dm.lib.irs_quasistatic_descent_workspace_bytes(dm.model_id, c["T"], 3) == 0        # they fit on chip
    on_chip = single_descend(dm, c)
    hbm = batch_descend(dm, [c], records_in_hbm=True)[0]
    certify(c, hbm, dm, "records in HBM")
    for k in hbm:
        np.testing.assert_array_equal(hbm[k].reshape(-1), on_chip[k].reshape(-1), err_msg=k)


# ------------------------------------------------------------------------------------------------ the host path
def hand_class(amd, c, **bounds):
    p = amd.IrsLqrQuasistaticParameters()
    q = {"sphere": np.array([1e-3, 1e-3, 10.0]), "arm_left": np.array([1e-3, 1e-3]),
         "arm_right": np.array([1e-3, 1e-3])}
    p.Q_dict, p.Qd_dict = q, {k: 10.0 * v for k, v in q.items()}
    p.R_dict = {"arm_left": 5.0 * np.ones(2), "arm_right": 5.0 * np.ones(2)}
    p.x0, p.x_trj_d, p.u_trj_0, p.T = c["x0"], c["xd"], c["u_trj"], c["T"]
    p.sampling = lambda u_initial, it: u_initial
    p.std_u_initial, p.num_samples, p.publish_every_iteration = 0.1 * np.ones(4), 300, False
    for k, v in bounds.items():
        setattr(p, k, v)
    sol = amd.IrsLqrQuasistatic(device_system(amd, "hand"), p)
    sol.verbose = False
    return sol


@pytest.mark.parametrize("kind", cc.KINDS)
def test_host_path_bound_arrays(amd, kind):
    """IrsLqrQuasistatic._bounds_dev with u_bounds_abs / u_bounds_rel as (2, T, m) arrays that hold infinities and as
    (2, m) per-component rows: the rows are orc.quasistatic_bounds' (which broadcasts the same way), and one
    local_descent of the class on the (2, T, m) array passes the tail-by-tail check on the data the class made."""
    from irs_mpc_amd import device as dev
    c = cc.case(cc.cid_of("hand", kind, "gaps", 11))
    T, m, idx = c["T"], c["m"], c["idx"]
    per_time = np.stack([c["off_lo"], c["off_hi"]])
    assert per_time.shape == (2, T, m) and np.isinf(per_time).any()
    one = cc.case(cc.cid_of("hand", kind, "one_sided", 11))
    per_comp = np.stack([one["off_lo"][0], one["off_hi"][0]])
    assert per_comp.shape == (2, m) and np.isinf(per_comp).any() and np.isfinite(per_comp).any()
    np.random.seed(5)                           # the class draws its perturbations as the reference does
    for b in (per_comp, per_time):
        sol = hand_class(amd, c, **{"u_bounds_" + kind: b})
        assert sol._solver == 3
        x_trj = np.asarray(sol.x_trj, float)
        rows = sol._bounds_dev(dev.to_dev(x_trj))
        want = orc.quasistatic_bounds(x_trj, idx, None, b if kind == "abs" else None, b if kind == "rel" else None)
        pair = (2, 3) if kind == "abs" else (4, 5)
        for i in range(6):
            if i in pair:
                assert tuple(rows[i].shape) == (T, m) and rows[i].is_contiguous()
                np.testing.assert_array_equal(rows[i].cpu().numpy(), want[i])
            else:
                assert rows[i] is None and not np.isfinite(want[i]).any()
        full = b if b.ndim == 3 else np.broadcast_to(b[:, None, :], (2, T, m))
        centre = x_trj[:-1, idx] if kind == "abs" else 0.0
        np.testing.assert_array_equal(want[pair[0]], centre + full[0])
        np.testing.assert_array_equal(want[pair[1]], centre + full[1])
    # the class's own descent on the per-time array: its sample pass makes (A, B, c), its rows are those above
    x_new, u_new, cost = sol._local_descent_dev(dev.to_dev(x_trj), dev.to_dev(np.asarray(sol.u_trj, float)))
    sol._check_last()
    out = dict(x_new=x_new.cpu().numpy(), u_new=u_new.cpu().numpy(), cost=cost.cpu().numpy(),
               info=sol._last["info"].cpu().numpy())
    made = cc.with_rows(c, want[pair[0]], want[pair[1]], x_trj=x_trj, x0=x_trj[0],
                        **{k: sol._last[k].cpu().numpy() for k in ("At", "Bt", "ct")})
    certify(made, out, sol._dm, "IrsLqrQuasistatic.local_descent")
