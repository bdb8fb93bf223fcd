"""The unbounded path's results on fixed inputs, to be held to the bits of the library as it stood when the Riccati
descent and the tail-plan test still had a single-problem and a batched kernel source each:

  * irs_tvlqr_descent per problem and irs_tvlqr_descent_batch on the smallest shapes that select each path of the
    backward pass (DESCENT_CASES), inputs from seeds through the generators of tests/test_irs_lqr_batch_gpu.py;
  * irs_tvlqr_descent on a contact model (planar hand, T = 8), whose inputs -- the oracle's zero-order linearisation
    along a rollout -- are stored in the fixture;
  * the four histories of irs_iterate in exact mode on the pendulum, T = 6, 3 descents (ITERATE_RUNS): without bounds
    (the info row comes from the descent's own launch), with +-1e4 bounds (from the plan test, flag 0) and with a u
    bound at 0.999 of the unbounded run's max |u| of descent 0 (flag 1).

results(amd, hand) runs them all; record() turns an array into its shape and the SHA-256 of its little-endian bytes
(and, for the short cases, its values, so that a mismatch can be located).  tests/golden/descent_parent_bits.json was
written by `python -m tests.helpers.descent_parent_cases OUT.json` with IRS_HIP_LIB naming that earlier library;
tests/test_descent_parent_bits_gpu.py requires the digests of the library in the tree to equal it."""
import ctypes
import hashlib
import json
import sys

import numpy as np
import torch

KEYS = ("K", "k", "x_new", "u_new", "cost", "info")
# (model, B, T, the backward pass it selects)
DESCENT_CASES = (("pendulum", 3, 5, "registers"), ("quadrotor", 3, 4, "matrix cores"), ("bicycle", 3, 4, "matrix cores"),
                 ("three_cart", 2, 4, "matrix cores"), ("quadrotor", 2, 341, "LDS recursion: (T + 1) 12 > 4096"))
HAND_T = 8
ITERATE_T, ITERATE_DESCENTS = 6, 3
ITERATE_RUNS = ("free", "wide", "u_cut")
VALUES_UP_TO_T = 8


def case_id(name, B, T):
    return "%s-B%d-T%d" % (name, B, T)


def npy(t):
    return t.detach().cpu().numpy()


def descent_inputs(name, B, T):
    """What test_descent_batch_equals_single_descents_bit_for_bit feeds the entries, without its bad problem."""
    from tests.test_irs_lqr_batch_gpu import model_problems, random_problems
    n, m = {"pendulum": (2, 1), "quadrotor": (12, 4), "bicycle": (5, 2), "three_cart": (6, 2)}[name]
    p = model_problems(name, 0.05, T, B) if T > 100 else random_problems(n, m, T, B, 0)
    rng = np.random.default_rng([n, m, T])
    p["Q"], p["Qd"] = np.diag(rng.uniform(0.5, 2.0, n)), np.diag(rng.uniform(5.0, 20.0, n))
    p["R"] = np.diag(rng.uniform(0.5, 2.0, m))
    return p


def run_descents(amd, name, B, T):
    """{"batch/<key>": array, "single/<b>/<key>": array}."""
    from irs_mpc_amd import device as dev
    from tests.test_irs_lqr_batch_gpu import device_system
    dm = device_system(amd, name).dm()
    d = {k: dev.to_dev(v) for k, v in descent_inputs(name, B, T).items()}
    got = dm.tvlqr_descent_batch(d["At"], d["Bt"], d["ct"], d["Q"], d["Qd"], d["R"], d["xd"], d["x0"])
    out = {"batch/" + key: npy(got[key]) for key in KEYS}
    for b in range(B):
        one = dm.tvlqr_descent(d["At"][b], d["Bt"][b], d["ct"][b], d["Q"], d["Qd"], d["R"], d["xd"][b],
                               d["x0"][b].contiguous())
        out.update({"single/%d/%s" % (b, key): npy(one[key]) for key in KEYS})
    return out


def hand_inputs():
    """The planar hand's problem (recording only; the test reads it from the fixture): the oracle's zero-order
    linearisation along the rollout of a random walk of joint commands from the example's settled start."""
    from oracle import irs_oracle as orc
    hand = orc.PlanarHandOracle
    rng = np.random.default_rng(HAND_T)
    sys_o = hand(0.1)
    u_hold = np.array([-np.pi / 4, -np.pi / 4, np.pi / 4, np.pi / 4])
    x0 = hand.pack([0.0, 0.35, 0.0], [-np.pi / 4, -np.pi / 4], [np.pi / 4, np.pi / 4])
    for _ in range(4):
        x0 = sys_o.dynamics(x0, u_hold)
    T = HAND_T
    u_trj = np.tile(x0[sys_o.indices_u_into_x], (T, 1)) + 0.03 * rng.normal(size=(T, 4)).cumsum(axis=0) / np.sqrt(T)
    x_trj = orc.rollout(sys_o, x0, u_trj)
    At, Bt, ct = orc.zero_order_B_decoupled(sys_o, x_trj, u_trj, 0.1 * rng.normal(size=(T, 300, 4)))
    Q = np.diag(hand.pack([1e-3, 1e-3, 10.0], [1e-3, 1e-3], [1e-3, 1e-3]))
    xd = np.tile(x0 + hand.pack([0.3, -0.1, 0.5], [0, 0], [0, 0]), (T + 1, 1))
    return dict(At=At, Bt=Bt, ct=ct, Q=Q, Qd=100.0 * Q, R=np.eye(4), xd=xd, x0=x0)


def run_hand(amd, inputs):
    from irs_mpc_amd import device as dev
    dm = amd.PlanarHandDynamics(0.1).dm()
    d = {k: dev.to_dev(np.asarray(v, float)) for k, v in inputs.items()}
    one = dm.tvlqr_descent(d["At"], d["Bt"], d["ct"], d["Q"], d["Qd"], d["R"], d["xd"], d["x0"])
    return {key: npy(one[key]) for key in KEYS}


def run_iterate(amd, ubound):
    """irs_iterate (exact linearisation) on the example's pendulum: {"x_hist", "u_hist", "cost_hist", "info_hist"}.
    ubound None: no bounds at all; else +-1e4 on x and +-ubound on u."""
    from examples.problems import pendulum
    from irs_mpc_amd import _lib, device as dev
    T, D = ITERATE_T, ITERATE_DESCENTS
    sysd, params, _, _, _ = pendulum(T)
    if ubound is None:
        params.xbound = params.ubound = None
    else:
        params.ubound = np.array([[-ubound], [ubound]])
    sol = amd.IrsLqrExact(sysd, params)
    n, m, dm = sol.dim_x, sol.dim_u, sol._dm
    c = _lib.IterateCall()
    dm.fill_call(c)
    c.mode, c.T, c.N, c.n_descents = _lib.ITERATE_EXACT, T, 0, D
    c.Q, c.Qd, c.R, c.xd_trj = (t_.data_ptr() for t_ in (sol._Q, sol._Qd, sol._R, sol._xd))
    c.alpha_R = 0.5
    box = sol._box_bounds()
    assert (box is None) == (ubound is None)
    if box is not None:
        c.xlo, c.xhi, c.ulo, c.uhi = (b.data_ptr() for b in box)
        c.qp_rho, c.qp_max_iter, c.qp_eps = 10.0, 5000, 1e-8
    x0d, u0d = dev.to_dev(np.asarray(sol.x_trj, float)), dev.to_dev(np.asarray(sol.u_trj, float))
    c.x_trj0, c.u_trj0 = x0d.data_ptr(), u0d.data_ptr()
    xh = torch.empty((D, T + 1, n), dtype=dev.F64, device="cuda")
    uh = torch.empty((D, T, m), dtype=dev.F64, device="cuda")
    ch = torch.empty((D,), dtype=dev.F64, device="cuda")
    ih = torch.zeros((D, 8), dtype=torch.int32, device="cuda")
    c.x_hist, c.u_hist, c.cost_hist, c.info_hist = xh.data_ptr(), uh.data_ptr(), ch.data_ptr(), ih.data_ptr()
    need = dm.lib.irs_iterate_scratch_bytes(dm.model_id, _lib.ITERATE_EXACT, T, 0)
    scratch = torch.empty((need,), dtype=torch.uint8, device="cuda")
    c.scratch, c.scratch_bytes = scratch.data_ptr(), scratch.numel()
    _lib.check(dm.lib.irs_iterate(ctypes.byref(c), None, dev._stream()), "irs_iterate")
    return dict(x_hist=npy(xh), u_hist=npy(uh), cost_hist=npy(ch), info_hist=npy(ih))


def run_iterates(amd):
    """{"iterate-<run>": histories} of ITERATE_RUNS; the cut is placed from the unbounded run."""
    free = run_iterate(amd, None)
    cut = 0.999 * float(np.abs(free["u_hist"][0]).max())
    return {"iterate-free": free, "iterate-wide": run_iterate(amd, 1e4), "iterate-u_cut": run_iterate(amd, cut)}


def results(amd, hand):
    """{case: {array name: array}} of everything above; `hand` is the planar hand's inputs."""
    out = {case_id(name, B, T): run_descents(amd, name, B, T) for name, B, T, _ in DESCENT_CASES}
    out["planar_hand-T%d" % HAND_T] = run_hand(amd, hand)
    out.update(run_iterates(amd))
    return out


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.astype(a.dtype.newbyteorder("<"), copy=False).tobytes()).hexdigest()


def record(a, values):
    r = dict(shape=list(a.shape), sha256=digest(a))
    if values:
        r["values"] = a.reshape(-1).tolist()
    return r


def short(case):
    """Whether the case's values are stored beside the digests (T <= VALUES_UP_TO_T)."""
    return not case.endswith("-T341")


if __name__ == "__main__":
    import irs_mpc_amd
    hand = hand_inputs()
    res = results(irs_mpc_amd, hand)
    # the values of a batched case once: those of the launch (its single descents are digests)
    gold = {case: {name: record(a, short(case) and not name.startswith("single/")) for name, a in arrays.items()}
            for case, arrays in res.items()}
    gold["planar_hand-T%d" % HAND_T]["inputs"] = {k: dict(shape=list(v.shape), values=v.reshape(-1).tolist())
                                                  for k, v in hand.items()}
    with open(sys.argv[1], "w") as f:
        json.dump(gold, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
