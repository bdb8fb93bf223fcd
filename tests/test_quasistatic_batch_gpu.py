"""B quasistatic descents in one launch (irs_quasistatic_box_descent_batch, IrsLqrQuasistaticBatch) against the
single-problem path.  Every problem of a batch runs the instructions of the single call on the same inputs, so
equality is bit for bit (torch.equal / assert_array_equal) everywhere; there is no tolerance in this file."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("x_new", "u_new", "cost", "info")


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return irs_mpc_amd


def descent_problem(make, T, B, kind, width, seed=11, N=512):
    """B descent problems of one task: distinct start states (small seeded offsets of the script's), distinct targets,
    per-problem (A, B, c) from the device sample pass on their own draws, and trust-region (abs) or rate (rel) rows."""
    from irs_mpc_amd import device as dev
    from irs_mpc_amd._lib import SMOOTH_ZERO_ORDER_B
    q_dynamics, x0, u0, Q_dict, Qd_dict, R_dict, xd = make(T, 0.1)
    dm, n, m = q_dynamics.dm(), q_dynamics.dim_x, q_dynamics.dim_u
    idx = torch.as_tensor(np.asarray(q_dynamics.get_u_indices_into_x()), device="cuda")
    Q, Qd, R = (dev.to_dev(np.asarray(a, float)) for a in (q_dynamics.get_Q_from_Q_dict(Q_dict),
                                                           q_dynamics.get_Q_from_Q_dict(Qd_dict),
                                                           q_dynamics.get_R_from_R_dict(R_dict)))
    rng = np.random.default_rng(seed)
    per = []
    for b in range(B):
        x0b = dev.to_dev(x0 + 1e-3 * rng.normal(size=n))
        xdb = dev.to_dev(xd + 0.05 * rng.normal(size=n))
        ub = dev.to_dev(u0)
        xb, _ = dm.rollout_cost(x0b, ub, Q, R, xdb)
        o = dm.smooth_rng(SMOOTH_ZERO_ORDER_B, xb, ub, N, None, [0.1] * m, seed + b, 1)
        assert not bool((o["info"] != 0).any().item())
        if kind == "abs":
            nom = xb[:-1].index_select(1, idx)
            lo, hi = (nom - width).contiguous(), (nom + width).contiguous()
        else:
            lo = torch.full((T, m), -width, dtype=torch.float64, device="cuda")
            hi = torch.full((T, m), width, dtype=torch.float64, device="cuda")
        per.append(dict(At=o["At"], Bt=o["Bt"], ct=o["ct"], xd=xdb, x0=xb[0].contiguous(), lo=lo, hi=hi))
    return dm, (Q, Qd, R), per, kind


def single_calls(dm, weights, per, kind, acts=None):
    """The oracle: one irs_quasistatic_box_descent_wsx (solver 3) per problem; returns the stacked outputs and sets."""
    outs, sets = [], []
    for b, q in enumerate(per):
        act = torch.zeros_like(q["lo"]) if acts is None else acts[b].clone()
        rows = dict(u_lo=q["lo"], u_hi=q["hi"]) if kind == "abs" else dict(du_lo=q["lo"], du_hi=q["hi"])
        o = dm.quasistatic_box_descent(q["At"], q["Bt"], q["ct"], *weights, q["xd"], q["x0"], solver=3, max_iter=2000,
                                       eps=1e-9, act=act, **rows)
        outs.append({k: o[k].clone() for k in KEYS})
        sets.append(act)
    stacked = {k: torch.stack([o[k] for o in outs]) for k in KEYS}
    stacked["cost"] = stacked["cost"].reshape(-1)
    return stacked, torch.stack(sets)


def batch_call(dm, weights, per, kind, acts=None, **kw):
    st = {k: torch.stack([q[k] for q in per]).contiguous() for k in per[0]}
    act = torch.zeros_like(st["lo"]) if acts is None else acts.clone()
    rows = dict(u_lo=st["lo"], u_hi=st["hi"]) if kind == "abs" else dict(du_lo=st["lo"], du_hi=st["hi"])
    o = dm.quasistatic_box_descent_batch(st["At"], st["Bt"], st["ct"], *weights, st["xd"], st["x0"], max_iter=2000,
                                         eps=1e-9, act=act, **rows, **kw)
    return o, act


def assert_same(got, want, got_act, want_act):
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got_act, want_act)


def check_cold_and_warm(dm, weights, per, kind, **kw):
    ref, ref_act = single_calls(dm, weights, per, kind)
    info = ref["info"].cpu().numpy()
    assert (info[:, 0] == 0).all() and (info[:, 2] == 0).all(), info
    # the bounds must bind, or the test shows nothing
    assert (info[:, 1] > 1).any(), info
    assert bool((ref_act != 0).any().item())
    got, got_act = batch_call(dm, weights, per, kind, **kw)
    assert_same(got, ref, got_act, ref_act)
    # again, every first tail starting from the set the previous descent returned
    ref2, ref_act2 = single_calls(dm, weights, per, kind, acts=ref_act)
    got2, got_act2 = batch_call(dm, weights, per, kind, acts=got_act, **kw)
    assert_same(got2, ref2, got_act2, ref_act2)
    return got, got_act


@pytest.fixture(scope="module")
def hand(amd):
    from examples.run_quasistatic import problem
    return descent_problem(problem, 10, 3, "abs", 0.05)


# ---------------------------------------------------------------- 1, 2: the descent, records on chip
def test_descent_batch_equals_single_calls_abs(hand):
    dm, weights, per, kind = hand
    assert dm.lib.irs_quasistatic_descent_batch_workspace_bytes(dm.model_id, 10, 3) == 0
    check_cold_and_warm(dm, weights, per, kind)


def test_descent_batch_equals_single_calls_rel(amd):
    from examples.run_quasistatic import box_problem
    dm, weights, per, kind = descent_problem(box_problem, 12, 3, "rel", 0.015)
    check_cold_and_warm(dm, weights, per, kind)


# ---------------------------------------------------------------- 3: records in HBM
def test_descent_batch_records_in_hbm_equal_on_chip(hand):
    dm, weights, per, kind = hand
    on_chip, act = batch_call(dm, weights, per, kind)
    got, got_act = check_cold_and_warm(dm, weights, per, kind, records_in_hbm=True)
    assert_same(got, on_chip, got_act, act)


def test_descent_batch_beyond_the_lds_horizon(amd):
    from examples.run_quasistatic import problem
    dm = problem(1, 0.1)[0].dm()
    ws_bytes = dm.lib.irs_quasistatic_descent_workspace_bytes
    T = next(t for t in range(1, 4096) if ws_bytes(dm.model_id, t, 3) > 0)      # the first horizon past the LDS cap
    assert ws_bytes(dm.model_id, T - 1, 3) == 0
    assert dm.lib.irs_quasistatic_descent_batch_workspace_bytes(dm.model_id, T, 2) > 0
    dm, weights, per, kind = descent_problem(problem, T, 2, "abs", 0.05)
    ref, ref_act = single_calls(dm, weights, per, kind)
    info = ref["info"].cpu().numpy()
    assert (info[:, 0] == 0).all() and (info[:, 2] == 0).all() and (info[:, 1] > 1).any(), info
    got, got_act = batch_call(dm, weights, per, kind)
    assert_same(got, ref, got_act, ref_act)


# ---------------------------------------------------------------- 4: more workgroups than compute units
def test_descent_batch_more_problems_than_compute_units(amd):
    from examples.run_quasistatic import problem
    B, T = 300, 6
    dm, weights, per, kind = descent_problem(problem, T, 1, "abs", 0.03)
    ref, ref_act = single_calls(dm, weights, per, kind)
    assert int(ref["info"][0, 1]) > 1 and bool((ref_act != 0).any().item())
    st = {k: per[0][k].unsqueeze(0).repeat(B, *([1] * per[0][k].dim())).contiguous() for k in per[0]}
    n, m = dm.n, dm.m
    out = dict(x_new=torch.full((B, T + 1, n), -7.0, dtype=torch.float64, device="cuda"),
               u_new=torch.full((B, T, m), -7.0, dtype=torch.float64, device="cuda"),
               cost=torch.full((B,), -7.0, dtype=torch.float64, device="cuda"),
               info=torch.full((B, 3), -7, dtype=torch.int32, device="cuda"))
    act = torch.zeros((B, T, m), dtype=torch.float64, device="cuda")
    dm.quasistatic_box_descent_batch(st["At"], st["Bt"], st["ct"], *weights, st["xd"], st["x0"], u_lo=st["lo"],
                                     u_hi=st["hi"], max_iter=2000, eps=1e-9, act=act, out=out)
    info = out["info"].cpu().numpy()
    assert (info != -7).all() and (info != -1).all(), "an info row was not written"
    for k in KEYS:
        want = ref[k][0]
        assert torch.equal(out[k], want.unsqueeze(0).expand(B, *want.shape)), k
    assert torch.equal(act, ref_act[0].unsqueeze(0).expand(B, T, m))


# ---------------------------------------------------------------- 5: bound rows
@pytest.mark.parametrize("per_time", [False, True])
def test_bound_rows_batch_equals_the_host_expression(amd, per_time):
    from examples.run_quasistatic import problem
    B, T = 3, 7
    q_dynamics = problem(T, 0.1)[0]
    dm, n, m = q_dynamics.dm(), q_dynamics.dim_x, q_dynamics.dim_u
    idx = torch.as_tensor(np.asarray(q_dynamics.get_u_indices_into_x()), device="cuda")
    g = torch.Generator(device="cuda").manual_seed(3)
    x_trj = torch.randn((B, T + 1, n), generator=g, device="cuda", dtype=torch.float64)
    off = torch.randn((B, 2, T, m) if per_time else (B, 2, m), generator=g, device="cuda", dtype=torch.float64) * 0.1
    off[0, 0].fill_(-float("inf"))                                  # an unbounded side stays unbounded
    lo, hi = dm.quasistatic_bound_rows_batch(x_trj, idx.to(torch.int32), off)
    rlo, rhi = dm.quasistatic_bound_rows_batch(x_trj, idx.to(torch.int32), off, rel=True)
    for b in range(B):
        # IrsLqrQuasistatic._bounds_dev
        center = x_trj[b][:-1].index_select(1, idx)
        assert torch.equal(lo[b], center + off[b, 0]) and torch.equal(hi[b], center + off[b, 1])
        zero = torch.zeros((T, m), dtype=torch.float64, device="cuda")
        assert torch.equal(rlo[b], zero + off[b, 0]) and torch.equal(rhi[b], zero + off[b, 1])


# ---------------------------------------------------------------- 6, 7: the class
def sampling(u_initial, it):
    return u_initial / (it ** 0.8)


def class_params(amd, make, T, B, mode, bounds, seed=5, N=512):
    q_dynamics, x0, u0, Q_dict, Qd_dict, R_dict, xd = make(T, 0.1)
    rng = np.random.default_rng(seed)
    m, ps = q_dynamics.dim_u, []
    for b in range(B):
        p = amd.IrsLqrQuasistaticParameters()
        p.Q_dict, p.Qd_dict, p.R_dict = Q_dict, Qd_dict, R_dict
        p.x0, p.T = x0, T
        p.x_trj_d = xd + 0.05 * rng.normal(size=q_dynamics.dim_x)
        p.u_trj_0 = u0 + 0.01 * rng.normal(size=u0.shape)
        w = (0.05, 0.04, 0.06)[b % 3]
        setattr(p, "u_bounds_" + bounds, np.array([-np.ones(m) * w, np.ones(m) * w]))
        p.sampling, p.std_u_initial, p.num_samples = sampling, np.ones(m) * 0.3, N
        p.gradient_mode, p.publish_every_iteration, p.device_rng_seed = mode, False, seed + b
        ps.append(p)
    return q_dynamics, ps


def run_single(amd, q_dynamics, p, iters):
    s = amd.IrsLqrQuasistatic(q_dynamics, p)
    s.verbose = False
    s.iterate(iters)
    return s


LISTS = ("x_trj_list", "u_trj_list", "cost_all_list", "cost_Qu_list", "cost_Qu_final_list", "cost_Qa_list",
         "cost_Qa_final_list", "cost_R_list")


def assert_problem_equals_single(batch, b, s):
    np.testing.assert_array_equal(batch.x_trj[b], s.x_trj)
    np.testing.assert_array_equal(batch.u_trj[b], s.u_trj)
    assert batch.cost[b] == s.cost
    for name in LISTS:
        got, want = getattr(batch, name)[b], getattr(s, name)
        assert len(got) == len(want), name
        for g, w in zip(got, want):
            np.testing.assert_array_equal(np.asarray(g), np.asarray(w), err_msg=name)
    assert batch.cost_best[b] == s.cost_best
    np.testing.assert_array_equal(batch.x_trj_best[b], s.x_trj_best)
    np.testing.assert_array_equal(batch.u_trj_best[b], s.u_trj_best)
    assert batch.problems[b].current_iter == s.current_iter


@pytest.mark.parametrize("system,mode,T,bounds", [("planar_hand", "zero_order_B", 10, "abs"),
                                                  ("box_pushing", "exact", 8, "rel")])
def test_class_equals_single_objects(amd, system, mode, T, bounds):
    from examples.run_quasistatic import problem, push_problem
    make = problem if system == "planar_hand" else push_problem
    q_dynamics, ps = class_params(amd, make, T, 3, mode, bounds)
    batch = amd.IrsLqrQuasistaticBatch(q_dynamics, ps)
    x, u, cost = batch.iterate(3)
    assert x.shape == (3, T + 1, q_dynamics.dim_x) and u.shape == (3, T, q_dynamics.dim_u) and cost.shape == (3,)
    assert batch.status == [None] * 3
    for b, p in enumerate(ps):
        s = run_single(amd, q_dynamics, p, 3)
        assert len(s.cost_all_list) == 5                     # the start and 3 + 1 descents
        assert_problem_equals_single(batch, b, s)
    assert len({float(c) for c in batch.cost}) == 3          # three different problems


def test_a_failed_problem_does_not_take_the_batch_down(amd):
    from examples.run_quasistatic import problem
    q_dynamics, ps = class_params(amd, problem, 10, 3, "zero_order_B", "abs")
    ps[1].std_u_initial = np.zeros(4)                        # no spread: the least squares for B is rank deficient
    for p in ps:
        p.qp_max_iter = 200          # shared; ample for a healthy T = 10 tail, and it bounds what the failed problem's
                                     # descents (on the output of a failed solve) can cost
    batch = amd.IrsLqrQuasistaticBatch(q_dynamics, ps)
    batch.iterate(3)
    with pytest.raises(ValueError) as err:
        run_single(amd, q_dynamics, ps[1], 3)
    assert batch.status[1] == str(err.value)
    assert batch.status[0] is None and batch.status[2] is None
    assert len(batch.cost_all_list[1]) == 1                  # nothing adopted, nothing logged after the start
    for b in (0, 2):
        assert_problem_equals_single(batch, b, run_single(amd, q_dynamics, ps[b], 3))


# ---------------------------------------------------------------- 8: the example
def test_example_script_runs_a_batch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_quasistatic.py"), "planar_hand", "irs_lqr",
                        "--T", "10", "--N", "500", "--iters", "2", "--batch", "3"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("problem ")]
    assert len(lines) == 3, r.stdout
    costs = [float(ln.split("final cost:")[1].split()[0]) for ln in lines]
    assert np.isfinite(costs).all() and len(set(costs)) == 3, costs
