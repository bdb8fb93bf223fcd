"""Device-resident CEM (csrc/cem.hip: candidates drawn inside the kernels, irs_cem_iterate) on the GPU.

The candidate stream is checked against its specification (oracle.irs_oracle.device_gaussian_samples); everything
else against the EXISTING kernels fed the materialised stream (irs_cem_candidates): the drawn rollout against
irs_cem_rollout_costs[_quasistatic], the drawn refit against irs_cem_refit, irs_cem_iterate against the composed loop of
those calls, and the public classes against that loop.  Shapes are the smallest that cross the 256- and 64-lane block
tails, T m across 64, n_elite below 16 and no multiple of 16, m = 1, 2, 4, a seed with high bits and a non-zero offset.
"""
import numpy as np
import pytest
import torch

from oracle import irs_oracle as orc

pytestmark = pytest.mark.gpu

SEED = 0x123456789ABC            # high bits set: both key words of the generator are used
OFFSET = 77


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()     # fails loudly if the HIP library is missing
    return irs_mpc_amd


def npy(t):
    return t.cpu().numpy()


def mean_std(T, m, seed):
    """Non-trivial (T,m) mean and positive std."""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(T, m)), 0.2 + rng.random(size=(T, m))


# ---------------------------------------------------------------- problems (carried here, not imported from a test)
def analytic_problem(name, T):
    """(system, x0, u0, Q, Qd, R, xd) of examples/problems.py."""
    from examples.problems import PROBLEMS
    sysd, p, _, _, _ = PROBLEMS[name](T)
    return sysd, p.x0, p.u_trj_initial, p.Q, p.Qd, p.R, p.xd_trj


def contact_problem(name, T):
    """Planar hand / box pivoting with the exact step QP (the classes' default), weights as matrices."""
    from examples import run_quasistatic as rq
    sd, x0, u0, Q_dict, Qd_dict, R_dict, xd = (rq.problem if name == "planar_hand" else rq.box_problem)(T)
    return sd, x0, u0, sd.get_Q_from_Q_dict(Q_dict), sd.get_Q_from_Q_dict(Qd_dict), sd.get_R_from_R_dict(R_dict), xd


def pendulum_cem_params(amd, T, B, n_elite, device_seed=None):
    p = amd.CemParameters()
    p.Q, p.Qd, p.R = np.diag([1., 1.]), np.diag([20., 20.]), np.diag([1.])
    p.x0 = np.array([0., 0.])
    p.xd_trj = np.tile(np.array([np.pi, 0.]), (T + 1, 1))
    p.u_trj_initial = np.tile(np.array([0.1]), (T, 1))
    p.initial_std = np.array([1.0])
    p.batch_size, p.n_elite = B, n_elite
    p.device_seed = device_seed
    return p


def box_cem_params(amd, T, B, n_elite, device_seed=None):
    from examples.run_quasistatic import box_problem
    sd, x0, u0, Q_dict, Qd_dict, R_dict, xd = box_problem(T)
    p = amd.CemQuasistaticParameters()
    p.Q_dict, p.Qd_dict, p.R_dict = Q_dict, Qd_dict, R_dict
    p.x0, p.xd_trj, p.u_trj_0, p.T = x0, xd, u0, T
    p.n_elite, p.batch_size, p.initial_std = n_elite, B, 0.1 * np.ones(2)
    p.publish_every_iteration = False
    p.device_seed = device_seed
    return sd, p


# ---------------------------------------------------------------- 1. the stream against its specification
STREAM = dict(T=5, B=300, it=4)


def stream_inputs(amd, m):
    from irs_mpc_amd import device as dev
    mean, std = mean_std(STREAM["T"], m, m)
    return amd.PendulumDynamics(0.05).dm(), mean, std, dev.to_dev(mean), dev.to_dev(std)   # any model: same stream


@pytest.mark.parametrize("m", [1, 2, 4])
def test_candidate_stream_matches_specification(amd, m):
    """cem_candidates = mean + std z, z the `du` stream of the smoothing generator with n = 0 and unit std.  The
    generator is f32, its restatement f64: rtol 2e-5 / atol 2e-6 on z (test_device_rng_matches_specification), i.e.
    std (2e-5 |z| + 2e-6) on u.

    The inputs include a pair with u1 = 1 - 1.28e-5 (candidate b = 77, t = 4, components 2 and 3 at m = 4): formed in f32
    as the smoothing generator forms it, its radius misses this bound by a factor 1.6, which is why the CEM stream takes
    that radius from 1 - u1 (philox_normal4<true>)."""
    dm, mean, std, mean_d, std_d = stream_inputs(amd, m)
    T, B, it = STREAM["T"], STREAM["B"], STREAM["it"]
    got = npy(dm.cem_candidates(mean_d, std_d, B, SEED, it, OFFSET))
    _, z = orc.device_gaussian_samples(T, B, 0, m, np.zeros(0), np.ones(m), SEED, it, OFFSET)
    z = z.transpose(1, 0, 2)
    assert got.shape == (B, T, m)
    err, tol = np.abs(got - (mean + std * z)), std * (2e-5 * np.abs(z) + 2e-6)
    print("m=%d: max |err| / tol = %.3g" % (m, (err / tol).max()))
    for b, t, j in zip(*np.nonzero(err > tol)):
        print("  over the bound: b=%d t=%d j=%d z=%.6g |err|/std=%.3g ratio=%.3g" % (
            b, t, j, z[b, t, j], err[b, t, j] / std[t, j], err[b, t, j] / tol[b, t, j]))
    assert (err <= tol).all()


@pytest.mark.parametrize("m", [1, 2, 4])
def test_candidate_stream_is_a_function_of_its_counters(amd, m):
    """A split by sample_offset reproduces the same rows bit for bit; the iteration is part of the counter."""
    dm, _, _, mean_d, std_d = stream_inputs(amd, m)
    B, it = STREAM["B"], STREAM["it"]
    got = npy(dm.cem_candidates(mean_d, std_d, B, SEED, it, OFFSET))
    part = npy(dm.cem_candidates(mean_d, std_d, 120, SEED, it, OFFSET + 180))
    np.testing.assert_array_equal(part, got[180:])
    other = npy(dm.cem_candidates(mean_d, std_d, B, SEED, it + 1, OFFSET))
    assert np.abs(other - got).max() > 0.1


# ---------------------------------------------------------------- 2. drawn rollout = supplied rollout
ROLLOUT_CASES = [("pendulum", 30, 0.5), ("quadrotor", 6, 0.05), ("bicycle", 8, 0.3), ("three_cart", 8, 0.3),
                 ("planar_hand", 8, 0.05), ("box_pivoting", 8, 0.1)]


@pytest.mark.parametrize("name,T,scale", ROLLOUT_CASES, ids=[c[0] for c in ROLLOUT_CASES])
def test_drawn_rollout_equals_supplied_rollout(amd, name, T, scale):
    """cem_rollout_costs[_quasistatic]_drawn against the existing kernel fed the output of cem_candidates: identical
    inputs, one shared body, so bit-equality is expected; asserted to rtol 1e-10 = f64 rounding (1.1e-16) x ~1e3
    operations of a step x T <= 30, with two decades for two instantiations scheduled differently."""
    from irs_mpc_amd import device as dev
    B, it = 300, 4
    contact = name in ("planar_hand", "box_pivoting")
    sd, x0, u0, Q, Qd, R, xd = (contact_problem if contact else analytic_problem)(name, T)
    dm = sd.dm()
    std = scale * (0.5 + np.random.default_rng(T).random(size=u0.shape))
    mean_d, std_d = dev.to_dev(np.asarray(u0, float)), dev.to_dev(std)
    x0_d, Q_d, Qd_d, R_d, xd_d = (dev.to_dev(np.asarray(a, float)) for a in (x0, Q, Qd, R, xd))
    cand = dm.cem_candidates(mean_d, std_d, B, SEED, it, OFFSET)
    if contact:
        want = npy(dm.cem_rollout_costs_quasistatic(cand, x0_d, Q_d, Qd_d, R_d, xd_d))
        got = npy(dm.cem_rollout_costs_quasistatic_drawn(mean_d, std_d, B, SEED, it, x0_d, Q_d, Qd_d, R_d, xd_d, OFFSET))
    else:
        want = npy(dm.cem_rollout_costs(cand, x0_d, Q_d, R_d, xd_d))
        got = npy(dm.cem_rollout_costs_drawn(mean_d, std_d, B, SEED, it, x0_d, Q_d, R_d, xd_d, OFFSET))
    assert np.isfinite(want).all() and want.std() > 0
    print("%s: max rel diff %.3g, bit-equal %s" % (name, np.abs(got / want - 1).max(), np.array_equal(got, want)))
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=0)


# ---------------------------------------------------------------- 3. drawn refit = refit on materialised candidates
@pytest.mark.parametrize("T,m,B,n_elite", [(30, 1, 300, 37), (20, 4, 300, 5), (5, 4, 64, 64), (17, 2, 300, 16)])
def test_drawn_refit_equals_refit_on_materialised_candidates(amd, T, m, B, n_elite):
    """Both refits get the SAME costs: identical elite_idx, u_new to rtol 1e-12 / atol 1e-13 and std_new to rtol 1e-9 /
    atol 1e-12 (the bounds test_cem_step_vs_oracle uses for the same sums)."""
    from irs_mpc_amd import device as dev
    it = 4
    mean, std = mean_std(T, m, 100 + T)
    mean_d, std_d = dev.to_dev(mean), dev.to_dev(std)
    dm = amd.PendulumDynamics(0.05).dm()
    costs = dev.to_dev(np.random.default_rng(B + n_elite).normal(size=B))
    cand = dm.cem_candidates(mean_d, std_d, B, SEED, it, OFFSET)
    idx0, u0, s0 = dm.cem_refit(cand, costs, n_elite)
    idx1, u1, s1 = dm.cem_refit_drawn(mean_d, std_d, SEED, it, costs, n_elite, OFFSET)
    np.testing.assert_array_equal(npy(idx1), npy(idx0))
    np.testing.assert_allclose(npy(u1), npy(u0), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(npy(s1), npy(s0), rtol=1e-9, atol=1e-12)
    # ... and NumPy on the materialised elites
    best = npy(cand)[npy(idx0)]
    np.testing.assert_allclose(npy(u1), best.mean(axis=0), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(npy(s1), best.std(axis=0), rtol=1e-9, atol=1e-12)
    np.testing.assert_array_equal(npy(mean_d), mean)        # the old mean / std are read, not written
    np.testing.assert_array_equal(npy(std_d), std)


def test_drawn_refit_ties_and_nan(amd):
    """The cost vector of test_cem_select_ties_and_nan through the drawn refit: equal costs at the threshold -- lowest
    indices win; NaN costs are never elite."""
    from irs_mpc_amd import device as dev
    dm = amd.PendulumDynamics(0.05).dm()
    costs = dev.to_dev(np.array([5., 1., 3., 3., np.nan, 3., 0.5, 3., 9., -2.]))
    mean_d, std_d = dev.to_dev(np.array([[0.3]])), dev.to_dev(np.array([[2.0]]))
    cand = npy(dm.cem_candidates(mean_d, std_d, 10, SEED, 1))
    idx, u_new, std_new = dm.cem_refit_drawn(mean_d, std_d, SEED, 1, costs, 5)
    assert sorted(npy(idx).tolist()) == [1, 2, 3, 6, 9]
    np.testing.assert_allclose(npy(u_new), cand[[1, 2, 3, 6, 9]].mean(axis=0), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(npy(std_new), cand[[1, 2, 3, 6, 9]].std(axis=0), rtol=1e-9, atol=1e-12)
    idx, _, _ = dm.cem_refit_drawn(mean_d, std_d, SEED, 1, costs, 9)
    assert 4 not in npy(idx).tolist()


# ---------------------------------------------------------------- 4. irs_cem_iterate = the composed loop
ITER_SEED = 20240521
_LOOPS = {}


def loop_problem(amd, name):
    """(dm, device tensors x0, Q, Qd, R, xd, u0, std0, B, n_elite, quasistatic) of the two iterate configurations."""
    from irs_mpc_amd import device as dev
    if name == "pendulum":
        p = pendulum_cem_params(amd, 30, 500, 25)
        sd, x0, u0, Q, Qd, R, xd, std0 = (amd.PendulumDynamics(0.05), p.x0, p.u_trj_initial, p.Q, p.Qd, p.R, p.xd_trj,
                                          np.tile(p.initial_std, (30, 1)))
        B, n_elite, qs = 500, 25, False
    else:
        sd, p = box_cem_params(amd, 8, 200, 10)
        x0, u0, xd, std0 = p.x0, p.u_trj_0, p.xd_trj, np.tile(p.initial_std, (8, 1))
        Q, Qd, R = sd.get_Q_from_Q_dict(p.Q_dict), sd.get_Q_from_Q_dict(p.Qd_dict), sd.get_R_from_R_dict(p.R_dict)
        B, n_elite, qs = 200, 10, True
    d = {k: dev.to_dev(np.asarray(v, float)) for k, v in dict(x0=x0, Q=Q, Qd=Qd, R=R, xd=xd, u0=u0, std0=std0).items()}
    return sd.dm(), d, B, n_elite, qs


def composed_loop(amd, name):
    """4 descents of cem_candidates -> cem_rollout_costs[_quasistatic] -> cem_refit -> rollout + cost on the existing
    kernels, generator iteration 1 + i; computed once per problem and shared (read only)."""
    if name in _LOOPS:
        return _LOOPS[name]
    dm, d, B, n_elite, qs = loop_problem(amd, name)
    mean, std = d["u0"], d["std0"]
    out = dict(u=[], std=[], x=[], cost=[], idx=[], costs=[], mean_in=[], std_in=[])
    for i in range(4):
        cand = dm.cem_candidates(mean, std, B, ITER_SEED, 1 + i)
        if qs:
            costs = dm.cem_rollout_costs_quasistatic(cand, d["x0"], d["Q"], d["Qd"], d["R"], d["xd"])
        else:
            costs = dm.cem_rollout_costs(cand, d["x0"], d["Q"], d["R"], d["xd"])
        idx, u_new, std_new = dm.cem_refit(cand, costs, n_elite)
        x_new, cost = dm.rollout_cost(d["x0"], u_new, d["Q"], d["R"], d["xd"])
        if qs:      # the mean is priced like the candidates
            cost = dm.cem_rollout_costs_quasistatic(u_new[None].contiguous(), d["x0"], d["Q"], d["Qd"], d["R"], d["xd"])
        out["mean_in"].append(mean)
        out["std_in"].append(std)
        for k, v in (("u", u_new), ("std", std_new), ("x", x_new), ("cost", cost), ("idx", idx), ("costs", costs)):
            out[k].append(npy(v))
        mean, std = u_new, std_new
    _LOOPS[name] = out
    return out


def assert_selection_is_well_separated(loop, n_elite):
    """Selection is discontinuous: a precondition on the INPUTS, for every descent -- the gap between the n_elite-th
    and the (n_elite+1)-th cost of the composed loop exceeds 1e-8 relative."""
    for i, costs in enumerate(loop["costs"]):
        c = np.sort(costs)
        assert np.isfinite(c).all()
        gap = (c[n_elite] - c[n_elite - 1]) / abs(c[n_elite - 1])
        print("descent %d: elite gap %.3g" % (i, gap))
        assert gap > 1e-8, (i, gap)


@pytest.mark.parametrize("name,k", [("pendulum", 4), ("box_pivoting", 3)])
def test_iterate_equals_the_composed_loop(amd, name, k):
    """irs_cem_iterate (one call, drawn kernels) against the loop of the existing calls on the materialised stream."""
    dm, d, B, n_elite, qs = loop_problem(amd, name)
    loop = composed_loop(amd, name)
    assert_selection_is_well_separated(loop, n_elite)
    o = dm.cem_iterate(d["u0"], d["std0"], d["x0"], d["Q"], d["Qd"], d["R"], d["xd"], B, n_elite, k, ITER_SEED, 1,
                       quasistatic=qs)
    # the elite sets of the drawn kernels, descent by descent, from the loop's own mean / std
    for i in range(k):
        mean, std = loop["mean_in"][i], loop["std_in"][i]
        if qs:
            costs = dm.cem_rollout_costs_quasistatic_drawn(mean, std, B, ITER_SEED, 1 + i, d["x0"], d["Q"], d["Qd"],
                                                           d["R"], d["xd"])
        else:
            costs = dm.cem_rollout_costs_drawn(mean, std, B, ITER_SEED, 1 + i, d["x0"], d["Q"], d["R"], d["xd"])
        idx, _, _ = dm.cem_refit_drawn(mean, std, ITER_SEED, 1 + i, costs, n_elite)
        assert sorted(npy(idx).tolist()) == sorted(loop["idx"][i].tolist()), i
    for key, hist in (("u", "u_hist"), ("std", "std_hist"), ("x", "x_hist"), ("cost", "cost_hist")):
        want = np.stack(loop[key][:k]).reshape(npy(o[hist]).shape)
        print("%s: max rel diff %.3g" % (hist, np.abs(npy(o[hist]) - want).max() / np.abs(want).max()))
        np.testing.assert_allclose(npy(o[hist]), want, rtol=1e-9, atol=0, err_msg=hist)


# ---------------------------------------------------------------- 5. the public classes
def forbid_host_candidates(monkeypatch, B, T, m):
    """np.random.normal and an upload of a (B,T,m) array raise: no host draw, no candidate tensor."""
    from irs_mpc_amd import device as dev

    def no_draw(*a, **k):
        raise AssertionError("np.random.normal called on the device-resident path")

    real = dev.to_dev

    def guarded(a, *args, **kw):
        if tuple(getattr(a, "shape", ())) == (B, T, m):
            raise AssertionError("a (B,T,m) candidate tensor was uploaded")
        return real(a, *args, **kw)

    monkeypatch.setattr(np.random, "normal", no_draw)
    monkeypatch.setattr(dev, "to_dev", guarded)


def test_cross_entropy_method_with_device_seed(amd, monkeypatch):
    loop = composed_loop(amd, "pendulum")
    assert_selection_is_well_separated(loop, 25)
    cem = amd.CrossEntropyMethod(amd.PendulumDynamics(0.05), pendulum_cem_params(amd, 30, 500, 25, ITER_SEED))
    cem.verbose = False
    forbid_host_candidates(monkeypatch, 500, 30, 1)
    x, u, cost = cem.iterate(3)
    assert len(cem.x_trj_lst) == len(cem.u_trj_lst) == len(cem.cost_lst) == 5 and cem.iter == 4
    for i in range(4):
        np.testing.assert_allclose(cem.u_trj_lst[1 + i], loop["u"][i], rtol=1e-9, atol=0)
        np.testing.assert_allclose(cem.x_trj_lst[1 + i], loop["x"][i], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(cem.cost_lst[1 + i], loop["cost"][i].item(), rtol=1e-9)
    np.testing.assert_allclose(cem.std_trj, loop["std"][3], rtol=1e-9, atol=0)
    # the last descent is logged but not adopted
    np.testing.assert_array_equal(u, cem.u_trj_lst[3])
    assert cost == cem.cost_lst[3] and cem.u_trj is u
    # local_descent continues the stream at self.iter around (u_trj, the carried std_trj), without a candidate tensor
    from irs_mpc_amd import device as dev
    it, mean, std = cem.iter, dev.to_dev(cem.u_trj), dev.to_dev(cem.std_trj)
    x_new, u_new = cem.local_descent(cem.x_trj, cem.u_trj)
    assert cem.iter == it and x_new.shape == (31, 2)
    costs = cem._dm.cem_rollout_costs_drawn(mean, std, 500, ITER_SEED, it, cem._x0, cem._Q, cem._R, cem._xd)
    idx, u_want, std_want = cem._dm.cem_refit_drawn(mean, std, ITER_SEED, it, costs, 25)
    np.testing.assert_array_equal(npy(cem.cost_array), npy(costs))
    np.testing.assert_array_equal(npy(cem.elite_idx), npy(idx))
    np.testing.assert_array_equal(u_new, npy(u_want))
    np.testing.assert_array_equal(cem.std_trj, npy(std_want))


def test_cross_entropy_method_quasistatic_with_device_seed(amd, monkeypatch):
    loop = composed_loop(amd, "box_pivoting")
    assert_selection_is_well_separated(loop, 10)
    sd, p = box_cem_params(amd, 8, 200, 10, ITER_SEED)
    sol = amd.CrossEntropyMethodQuasistatic(sd, p)
    sol.verbose = False
    forbid_host_candidates(monkeypatch, 200, 8, 2)
    x, u, cost = sol.iterate(3)
    assert len(sol.x_trj_list) == len(sol.u_trj_list) == len(sol.cost_all_list) == len(sol.cost_R_list) == 5
    assert sol.current_iter == 4 and sol.cost_best == min(sol.cost_all_list[1:])
    for i in range(4):
        np.testing.assert_allclose(sol.u_trj_list[1 + i], loop["u"][i], rtol=1e-9, atol=0)
        np.testing.assert_allclose(sol.x_trj_list[1 + i], loop["x"][i], rtol=1e-9, atol=1e-12)
        # the five-term host log and the device's candidate cost are the same function
        np.testing.assert_allclose(sol.cost_all_list[1 + i], loop["cost"][i].item(), rtol=1e-9)
    np.testing.assert_allclose(sol.std_trj, loop["std"][3], rtol=1e-9, atol=0)
    np.testing.assert_array_equal(u, sol.u_trj_list[3])
    # local_descent continues the stream at current_iter around (u_trj, the carried std_trj)
    from irs_mpc_amd import device as dev
    it, mean, std = sol.current_iter, dev.to_dev(sol.u_trj), dev.to_dev(sol.std_trj)
    x_new, u_new = sol.local_descent(sol.x_trj, sol.u_trj)
    costs = sol._dm.cem_rollout_costs_quasistatic_drawn(mean, std, 200, ITER_SEED, it, sol._x0, sol._Q, sol._Qd, sol._R,
                                                        sol._xd)
    idx, u_want, std_want = sol._dm.cem_refit_drawn(mean, std, ITER_SEED, it, costs, 10)
    np.testing.assert_array_equal(npy(sol.cost_array), npy(costs))
    np.testing.assert_array_equal(npy(sol.elite_idx), npy(idx))
    np.testing.assert_array_equal(u_new, npy(u_want))
    np.testing.assert_array_equal(sol.std_trj, npy(std_want))


def test_device_seed_cem_reduces_cost_on_the_pendulum(amd):
    """The configuration of test_cem_iterate_reduces_cost.  (Strict monotonicity there is a property of that test's
    NumPy seed, not of CEM: not asserted for this stream.)"""
    cem = amd.CrossEntropyMethod(amd.PendulumDynamics(0.05), pendulum_cem_params(amd, 30, 2000, 20, 0))
    cem.verbose = False
    cem.iterate(5)
    assert len(cem.cost_lst) == 7 and np.isfinite(cem.cost_lst).all()
    print("cost history", cem.cost_lst)
    assert cem.cost_lst[-1] < cem.cost_lst[0]


def test_without_device_seed_the_host_draw_is_unchanged(amd):
    """device_seed = None: local_descent under np.random.seed(s) returns what the host-draw path always did -- the
    existing kernels on np.random.normal candidates of the same seed."""
    from irs_mpc_amd import device as dev
    T, B, n_elite = 30, 300, 37
    p = pendulum_cem_params(amd, T, B, n_elite)
    cem = amd.CrossEntropyMethod(amd.PendulumDynamics(0.05), p)
    np.random.seed(11)
    x_new, u_new = cem.local_descent(cem.x_trj, cem.u_trj)
    np.random.seed(11)
    cand = dev.to_dev(np.random.normal(p.u_trj_initial, np.tile(p.initial_std, (T, 1)), (B, T, 1)))
    dm = amd.PendulumDynamics(0.05).dm()
    x0, Q, R, xd = (dev.to_dev(np.asarray(a, float)) for a in (p.x0, p.Q, p.R, p.xd_trj))
    costs = dm.cem_rollout_costs(cand, x0, Q, R, xd)
    idx, u_mean, u_std = dm.cem_refit(cand, costs, n_elite)
    x_mean, _ = dm.rollout_cost(x0, u_mean, Q, R, xd)
    np.testing.assert_array_equal(u_new, npy(u_mean))
    np.testing.assert_array_equal(cem.std_trj, npy(u_std))
    np.testing.assert_array_equal(x_new, npy(x_mean))
    np.testing.assert_array_equal(npy(cem.cost_array), npy(costs))
    np.testing.assert_array_equal(npy(cem.elite_idx), npy(idx))
    # a parameter object written for the reference has no device_seed attribute at all
    del p.device_seed
    assert amd.CrossEntropyMethod(amd.PendulumDynamics(0.05), p).device_seed is None
    # the quasistatic class
    sd, pq = box_cem_params(amd, 8, 200, 10)
    sol = amd.CrossEntropyMethodQuasistatic(sd, pq)
    np.random.seed(12)
    xq, uq = sol.local_descent(sol.x_trj, sol.u_trj)
    np.random.seed(12)
    cand = dev.to_dev(np.random.normal(pq.u_trj_0, np.tile(pq.initial_std, (8, 1)), (200, 8, 2)))
    costs = sd.dm().cem_rollout_costs_quasistatic(cand, sol._x0, sol._Q, sol._Qd, sol._R, sol._xd)
    _, u_mean, u_std = sd.dm().cem_refit(cand, costs, 10)
    np.testing.assert_array_equal(uq, npy(u_mean))
    np.testing.assert_array_equal(sol.std_trj, npy(u_std))


@pytest.mark.parametrize("module,argv", [("examples.run", ["pendulum", "cem", "--iters", "2", "--T", "40", "--quiet",
                                                           "--device-rng"]),
                                         ("examples.run_quasistatic", ["planar_hand", "cem", "--iters", "2", "--T", "8",
                                                                       "--N", "60", "--quiet", "--device-rng"])])
def test_example_runners_take_device_rng_for_cem(amd, module, argv, monkeypatch, capsys):
    import importlib
    run = importlib.import_module(module)
    forbid_host_candidates(monkeypatch, -1, -1, -1)         # no host draw at all
    monkeypatch.setattr("sys.argv", ["run.py"] + argv)
    run.main()
    hist = [float(v) for v in capsys.readouterr().out.split("cost history:")[1].split()]
    assert len(hist) == 4 and all(np.isfinite(hist))


# ---------------------------------------------------------------- 6. one candidate source under both device models
def test_candidate_source_primitives_on_a_torch_system(amd):
    """cem_costs / cem_refit_from on a TorchDeviceModel with a CemSource of a non-zero sample_offset, which the public
    classes never pass.  The drawn source against the supplied source on the materialised stream: costs and elite_idx
    under torch.equal (one candidate stream, one cost body, as test_drawn_stage_equals_supplied_stage holds stage by
    stage), the refit to the bounds of test_drawn_refit_equals_refit_on_materialised_candidates.  The public names are
    the primitives; the quasistatic cost is refused as cem_iterate(quasistatic=True) refuses it.  B = 300: the third
    128-lane stage workgroup is ragged."""
    from examples.torch_systems import TorchPendulum
    from irs_mpc_amd import device as dev
    T, B, n_elite, it = 3, 300, 7, 4
    dm = TorchPendulum(0.05).dm()
    mean, std = mean_std(T, 1, 3)
    mean_d, std_d = dev.to_dev(mean), dev.to_dev(std)
    x0, Q, R = dev.to_dev(np.zeros(2)), dev.to_dev(np.diag([1., 2.])), dev.to_dev(np.eye(1))
    xd = dev.to_dev(np.tile(np.array([np.pi, 0.]), (T + 1, 1)))
    drawn = dev.CemSource.drawn(mean_d, std_d, B, SEED, it, OFFSET)
    supplied = dev.CemSource.supplied(dm.cem_candidates(mean_d, std_d, B, SEED, it, OFFSET))
    assert (drawn.B, drawn.T, drawn.m) == (supplied.B, supplied.T, supplied.m) == (B, T, 1)
    c_drawn, c_sup = dm.cem_costs(drawn, x0, Q, R, xd), dm.cem_costs(supplied, x0, Q, R, xd)
    assert np.isfinite(npy(c_sup)).all() and float(c_sup.std()) > 0
    assert torch.equal(c_drawn, c_sup)
    assert torch.equal(dm.cem_rollout_costs_drawn(mean_d, std_d, B, SEED, it, x0, Q, R, xd, OFFSET), c_drawn)
    assert not torch.equal(dm.cem_rollout_costs_drawn(mean_d, std_d, B, SEED, it, x0, Q, R, xd), c_drawn)   # offset 0
    assert torch.equal(dm.cem_rollout_costs(supplied.tensors[0], x0, Q, R, xd), c_sup)
    idx1, u1, s1 = dm.cem_refit_from(drawn, c_drawn, n_elite)
    idx0, u0, s0 = dm.cem_refit_from(supplied, c_sup, n_elite)
    assert torch.equal(idx1, idx0)
    np.testing.assert_allclose(npy(u1), npy(u0), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(npy(s1), npy(s0), rtol=1e-9, atol=1e-12)
    for call in (lambda: dm.cem_costs(drawn, x0, Q, R, xd, Qd=Q),
                 lambda: dm.cem_rollout_costs_quasistatic(supplied.tensors[0], x0, Q, Q, R, xd)):
        with pytest.raises(NotImplementedError, match="compiled position-controlled model"):
            call()
