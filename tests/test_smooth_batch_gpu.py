"""The sample passes of B problems in one launch (irs_smooth_rng_batch, DeviceModel.smooth_rng_batch, the
`batched_sample_pass` path of IrsLqrQuasistaticBatch) against one single-problem call per problem on the same inputs.
Row (b, t) of the batched launch runs the instructions of the single call on problem b -- the same launch geometry,
draws and summation order -- so equality is bit for bit (torch.equal / assert_array_equal) everywhere; there is no
tolerance in this file."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("sums", "At", "Bt", "ct", "info")
ZERO_ORDER_B, FIRST_ORDER = 2, 1
MODES = [ZERO_ORDER_B, FIRST_ORDER]


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return irs_mpc_amd


class Problems:
    """B problems of one task, built as the descent problems of test_quasistatic_batch_gpu.py: the script's start
    state plus seeded 1e-3 offsets, rolled out under the script's commands (plus a small seeded offset per problem),
    with distinct seeds -- one with its top bit set: the seeds travel as uint64 bits -- and distinct std_u."""

    def __init__(self, make, T, B, seed=11):
        from irs_mpc_amd import device as dev
        q_dynamics, x0, u0, Q_dict, _, R_dict, xd = make(T, 0.1)
        self.dm, self.T, self.B = q_dynamics.dm(), T, B
        n, m = q_dynamics.dim_x, q_dynamics.dim_u
        Q, R = (dev.to_dev(np.asarray(a, float)) for a in (q_dynamics.get_Q_from_Q_dict(Q_dict),
                                                           q_dynamics.get_R_from_R_dict(R_dict)))
        rng = np.random.default_rng(seed)
        xs, us = [], []
        for b in range(B):
            ub = dev.to_dev(u0 + 1e-3 * rng.normal(size=u0.shape))
            xb, _ = self.dm.rollout_cost(dev.to_dev(x0 + 1e-3 * rng.normal(size=n)), ub, Q, R, dev.to_dev(xd))
            xs.append(xb)
            us.append(ub)
        self.X, self.U = torch.stack(xs).contiguous(), torch.stack(us).contiguous()      # (B,T+1,n), (B,T,m)
        self.std = 0.05 + 0.1 * rng.random((B, m))
        self.seeds = [seed + 1000 * b for b in range(B)]
        self.seeds[-1] |= 1 << 63

    def pick(self, order):
        """The same problems in another order (a view of this object's data, copied)."""
        q = object.__new__(Problems)
        q.dm, q.T, q.B = self.dm, self.T, len(order)
        q.X, q.U = self.X[order].contiguous(), self.U[order].contiguous()
        q.std, q.seeds = self.std[order].copy(), [self.seeds[i] for i in order]
        return q


def singles(p, mode, N, it=1):
    """The reference: one dm.smooth_rng per problem, stacked."""
    outs = []
    for b in range(p.B):
        o = p.dm.smooth_rng(mode, p.X[b], p.U[b], N, None, list(p.std[b]), p.seeds[b], it)
        outs.append({k: o[k].clone() for k in KEYS})
    return {k: torch.stack([o[k] for o in outs]) for k in KEYS}


def batched(p, mode, N, it=1, X=None, out=None):
    from irs_mpc_amd import device as dev
    seeds = torch.as_tensor(np.array(p.seeds, dtype=np.uint64).view(np.int64)).cuda()
    return p.dm.smooth_rng_batch(mode, p.X if X is None else X, p.U, N, dev.to_dev(p.std), seeds, it, out=out)


def assert_reference_shows_something(ref, healthy=None):
    """What every test asserts first: the single calls solved every healthy problem, and the problems differ -- a
    mixed-up problem index would not pass."""
    info = ref["info"] if healthy is None else ref["info"][healthy]
    assert not bool((info != 0).any().item()), ref["info"].cpu().numpy()
    assert any(not torch.equal(ref["Bt"][0], ref["Bt"][b]) for b in range(1, ref["Bt"].shape[0]))


def assert_same(got, want):
    for k in KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert torch.equal(got[k], want[k]), k


_cache = {}


def hand_case(T, B, N, mode):
    """Planar-hand problems and their single-call reference, computed once per (T, B, N, mode) and left unchanged."""
    from examples.run_quasistatic import problem
    if ("p", T, B) not in _cache:
        _cache[("p", T, B)] = Problems(problem, T, B)
    p = _cache[("p", T, B)]
    if (T, B, N, mode) not in _cache:
        _cache[(T, B, N, mode)] = singles(p, mode, N)
    return p, _cache[(T, B, N, mode)]


# ---------------------------------------------------------------- 1: one partial block, one workgroup per row
@pytest.mark.parametrize("mode", MODES)
def test_planar_hand_one_workgroup_per_row(amd, mode):
    p, ref = hand_case(4, 3, 100, mode)
    assert_reference_shows_something(ref)
    g = p.dm.smooth_geometry(mode, 4, 100, rng=True)
    assert g["family"] == "uniform_geometry" and g["nblk"] == 1
    assert_same(batched(p, mode, 100), ref)


# ---------------------------------------------------------------- 2: the ticket path, three rounds of blocks
@pytest.mark.parametrize("mode", MODES)
def test_planar_hand_several_workgroups_per_row(amd, mode):
    T, N = 64, 4200
    p, ref = hand_case(T, 3, N, mode)
    assert_reference_shows_something(ref)
    g = p.dm.smooth_geometry(mode, T, N, rng=True)
    assert g["family"] == "uniform_geometry" and g["nblk"] >= 2
    assert -(-N // 64) > 2 * (8 * g["nblk"] - 1), g       # a third round, which the nominal wave joins
    assert N % 64 != 0                                    # a partial last block
    assert_same(batched(p, mode, N), ref)


# ---------------------------------------------------------------- 3: more rows than a slice has counters, than CUs
def test_rows_beyond_one_slice_of_counters(amd):
    B, T, N, mode = 40, 30, 64, ZERO_ORDER_B
    p, ref = hand_case(T, B, N, mode)
    assert_reference_shows_something(ref)
    assert B * T > 1024
    n, m, P = p.dm.n, p.dm.m, p.dm.sums_len(mode)
    out = dict(sums=torch.full((B, T, P), -7.0, dtype=torch.float64, device="cuda"),
               At=torch.full((B, T, n, n), -7.0, dtype=torch.float64, device="cuda"),
               Bt=torch.full((B, T, n, m), -7.0, dtype=torch.float64, device="cuda"),
               ct=torch.full((B, T, n), -7.0, dtype=torch.float64, device="cuda"),
               info=torch.full((B, T), -7, dtype=torch.int32, device="cuda"))
    got = batched(p, mode, N, out=out)
    assert got is out
    assert not bool((out["info"] == -7).any().item()), "an info row was not written"
    for k in ("sums", "Bt", "ct"):                        # (At holds no -7 either: its entries are 0 and 1)
        assert not bool((out[k] == -7.0).any().item()), k
    assert_same(out, ref)


# ---------------------------------------------------------------- 4: strides, order
@pytest.mark.parametrize("mode", MODES)
def test_strides_and_problem_order(amd, mode):
    p, ref = hand_case(4, 3, 100, mode)
    assert_reference_shows_something(ref)
    points = p.X[:, :-1, :].contiguous()                  # (B,T,n): stacked nominal points, stride T n
    assert points.stride(0) == 4 * p.dm.n and p.X.stride(0) == 5 * p.dm.n
    assert_same(batched(p, mode, 100, X=points), ref)
    assert_same(batched(p, mode, 100), ref)
    view = p.X[:, :-1, :]                                 # the trajectory tensor's first T rows, not contiguous as a whole
    assert not view.is_contiguous()
    assert_same(batched(p, mode, 100, X=view), ref)
    rev = p.pick([2, 1, 0])
    assert_same(batched(rev, mode, 100), {k: ref[k].flip(0) for k in KEYS})


# ---------------------------------------------------------------- 5: iteration counter, workspace reuse
def test_iteration_counter_and_workspace_reuse(amd):
    mode, T, N = ZERO_ORDER_B, 4, 100
    p, ref1 = hand_case(T, 3, N, mode)
    assert_reference_shows_something(ref1)
    ref3 = singles(p, mode, N, it=3)
    assert_reference_shows_something(ref3)
    assert not torch.equal(ref1["Bt"], ref3["Bt"])
    got1 = {k: v.clone() for k, v in batched(p, mode, N, it=1).items()}
    ws = p.dm._ws[(("smooth_batch", mode, T, N), p.X.device)]
    got3 = {k: v.clone() for k, v in batched(p, mode, N, it=3).items()}
    assert_same(got1, ref1)
    assert_same(got3, ref3)
    assert not torch.equal(got1["Bt"], got3["Bt"])
    two = p.pick([0, 1])
    got2 = batched(two, mode, N, it=3)
    assert p.dm._ws[(("smooth_batch", mode, T, N), p.X.device)] is ws          # the same, larger, workspace
    assert_same(got2, {k: ref3[k][:2] for k in KEYS})
    # every call left all arrival counters zero: the head of each slice
    stride = (p.dm.lib.irs_smooth_workspace_bytes(p.dm.model_id, mode, T, N) + 255) // 256 * 256
    for b in range(3):
        assert not bool(ws[b * stride: b * stride + 4096].any().item()), b


# ---------------------------------------------------------------- 6: a failed problem stays alone
def test_a_rank_deficient_problem_does_not_touch_its_neighbours(amd):
    mode, T, N = ZERO_ORDER_B, 4, 100
    base, _ = hand_case(T, 3, N, mode)
    p = base.pick([0, 1, 2])
    p.std[1] = 0.0                                        # no spread: the least squares for B is rank deficient
    ref = singles(p, mode, N)
    assert_reference_shows_something(ref, healthy=[0, 2])
    assert bool((ref["info"][1] != 0).all().item())
    got = batched(p, mode, N)
    assert torch.equal(got["info"], ref["info"])
    assert not bool((got["info"][[0, 2]] != 0).any().item())
    for b in (0, 2):
        for k in KEYS:
            assert torch.equal(got[k][b], ref[k][b]), (b, k)
    assert torch.equal(got["sums"][1], ref["sums"][1])


# ---------------------------------------------------------------- 7: the general kernel is refused, not approximated
def test_general_kernel_is_refused(amd, monkeypatch):
    """The general kernel has no batched form (its compiled code did not stay bit-equal behind a problem index): the
    models it serves, and the planar hand once IRS_UG=0 selects it, are refused before anything is launched."""
    from examples.run_quasistatic import box_problem, push_problem
    for make in (box_problem, push_problem):
        p = Problems(make, 5, 3)
        for mode in MODES:
            assert not p.dm.smooth_batch_supported(mode)
            with pytest.raises(NotImplementedError):
                batched(p, mode, 100)
    p, ref = hand_case(4, 3, 100, ZERO_ORDER_B)
    monkeypatch.setenv("IRS_UG", "0")                     # read per call
    assert p.dm.smooth_geometry(ZERO_ORDER_B, 4, 100, rng=True)["family"] == "contact_parked"
    assert not p.dm.smooth_batch_supported(ZERO_ORDER_B)
    with pytest.raises(NotImplementedError):
        batched(p, ZERO_ORDER_B, 100)
    monkeypatch.delenv("IRS_UG")
    assert_same(batched(p, ZERO_ORDER_B, 100), ref)


# ---------------------------------------------------------------- 8: the class
def sampling(u_initial, it):
    return u_initial / (it ** 0.8)


LISTS = ("x_trj_list", "u_trj_list", "cost_all_list", "cost_Qu_list", "cost_Qu_final_list", "cost_Qa_list",
         "cost_Qa_final_list", "cost_R_list")


def class_params(amd, system, mode, bounds, T=10, B=3, N=512):
    from examples.run_quasistatic import box_problem, problem
    served = system == "planar_hand"
    q_dynamics, x0, u0, Q_dict, Qd_dict, R_dict, xd = (problem if served else box_problem)(T, 0.1)
    rng = np.random.default_rng(5)
    m, ps = q_dynamics.dim_u, []
    for b in range(B):
        p = amd.IrsLqrQuasistaticParameters()
        p.Q_dict, p.Qd_dict, p.R_dict = Q_dict, Qd_dict, R_dict
        p.x0, p.T = x0, T
        p.x_trj_d = xd + 0.05 * rng.normal(size=q_dynamics.dim_x)
        p.u_trj_0 = u0 + 0.01 * rng.normal(size=u0.shape)
        # the scripts' widths and spreads (+-0.5 h absolute / +-0.15 h on the rate; std 0.3 / 0.1), varied per problem
        w = ((0.05, 0.04, 0.06) if bounds == "abs" else (0.015, 0.012, 0.018))[b]
        setattr(p, "u_bounds_" + bounds, np.array([-np.ones(m) * w, np.ones(m) * w]))
        std0 = (0.3 if served else 0.1) * (1.0, 0.8, 0.6)[b]
        p.sampling, p.std_u_initial, p.num_samples = sampling, np.ones(m) * std0, N
        p.gradient_mode, p.publish_every_iteration, p.device_rng_seed = mode, False, 5 + b
        ps.append(p)
    return q_dynamics, ps


def count_calls(dm, monkeypatch):
    calls = dict(batch=0, single=0)

    def count(name, fn):
        def wrapped(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapped

    monkeypatch.setattr(dm, "smooth_rng_batch", count("batch", dm.smooth_rng_batch))
    monkeypatch.setattr(dm, "smooth_rng", count("single", dm.smooth_rng))
    return calls


@pytest.mark.parametrize("system,mode,bounds", [("planar_hand", "zero_order_B", "abs"),
                                                ("planar_hand", "first_order", "abs"),
                                                ("box_pivoting", "first_order", "rel")])
def test_class_batched_pass_equals_the_loop(amd, system, mode, bounds, monkeypatch):
    """`batched_sample_pass=True` against `False`: one smooth_rng_batch call per descent and no single call where the
    batched pass serves the model (the planar hand); where it does not (box pivoting: the general kernel) the keyword
    resolves to False and the object runs the loop -- the same bits either way."""
    B, served = 3, system == "planar_hand"
    q_dynamics, ps = class_params(amd, system, mode, bounds)
    calls = count_calls(q_dynamics.dm(), monkeypatch)
    on = amd.IrsLqrQuasistaticBatch(q_dynamics, ps, batched_sample_pass=True)
    assert on.batched_sample_pass == served
    on.iterate(3)
    first = dict(batch=4, single=0) if served else dict(batch=0, single=4 * B)      # 3 + 1 descents
    assert calls == first
    off = amd.IrsLqrQuasistaticBatch(q_dynamics, ps, batched_sample_pass=False)
    assert not off.batched_sample_pass
    off.iterate(3)
    assert calls == dict(batch=first["batch"], single=first["single"] + 4 * B)
    assert on.status == off.status == [None] * B
    assert len({float(c) for c in on.cost}) == B          # three different problems
    np.testing.assert_array_equal(on.x_trj, off.x_trj)
    np.testing.assert_array_equal(on.u_trj, off.u_trj)
    np.testing.assert_array_equal(on.cost, off.cost)
    np.testing.assert_array_equal(on.cost_best, off.cost_best)
    for b in range(B):
        for name in LISTS:
            got, want = getattr(on, name)[b], getattr(off, name)[b]
            assert len(got) == len(want) == 5, name           # the start and 3 + 1 descents
            for g, w in zip(got, want):
                np.testing.assert_array_equal(np.asarray(g), np.asarray(w), err_msg=name)
        np.testing.assert_array_equal(on.x_trj_best[b], off.x_trj_best[b])
        np.testing.assert_array_equal(on.u_trj_best[b], off.u_trj_best[b])
        assert on.problems[b].current_iter == off.problems[b].current_iter


def test_class_falls_back_when_the_general_kernel_is_selected_later(amd, monkeypatch):
    """IRS_UG is read per call: set to 0 after the object exists, the planar hand's passes go to the general kernel,
    which has no batched form -- the object runs the loop (it does not raise) and computes what the loop computes."""
    B = 3
    q_dynamics, ps = class_params(amd, "planar_hand", "zero_order_B", "abs")
    calls = count_calls(q_dynamics.dm(), monkeypatch)
    on = amd.IrsLqrQuasistaticBatch(q_dynamics, ps, batched_sample_pass=True)
    assert on.batched_sample_pass
    monkeypatch.setenv("IRS_UG", "0")
    on.iterate(1)
    assert calls == dict(batch=0, single=2 * B)           # 1 + 1 descents
    off = amd.IrsLqrQuasistaticBatch(q_dynamics, ps, batched_sample_pass=False)
    off.iterate(1)
    assert on.status == off.status == [None] * B
    np.testing.assert_array_equal(on.x_trj, off.x_trj)
    np.testing.assert_array_equal(on.u_trj, off.u_trj)
    np.testing.assert_array_equal(on.cost, off.cost)
