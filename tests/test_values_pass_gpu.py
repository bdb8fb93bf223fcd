"""GPU tests of the bring-your-own-dynamics path: the values pass (csrc/smooth_values.hip) against the f64 NumPy
statement on identical f32 inputs (tests/helpers/values_cases.py; the inputs are certified on the CPU in
tests/test_values_pass_cpu.py), and TorchDynamicalSystem through the three optimiser classes against the compiled
pendulum, the reference's own recorded results and the NumPy oracle on a system that has no device functor.

Tolerance: the sample pass's stated TOL_AB (tests/test_gpu_parity.py).  The statistics themselves are held
to a rounding bound: every entry is an f32 chain of at most 1024 products before it moves to f64, so its error is at
most 1025 * 2^-24 of the sum of the absolute values of its terms.
"""
import os

import numpy as np
import pytest
import torch

import irs_mpc_amd as pkg
from oracle import irs_oracle as orc
from tests.helpers import values_cases as vc

pytestmark = pytest.mark.gpu

TOL_AB = dict(rtol=1e-4, atol=2e-5)
SUMS_BOUND = 1025 * 2.0 ** -24


@pytest.fixture(scope="module")
def amd():
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()     # fails loudly if the HIP library is missing
    return pkg


def on_device(c):
    from irs_mpc_amd import device as dev
    f32 = {k: dev.to_dev(c[k], dev.F32) for k in ("dx", "du", "fz", "f0")}
    f64 = {k: dev.to_dev(c[k]) for k in ("x_trj", "u_trj", "fnom")}
    return f32, f64


def run_fused(c):
    from irs_mpc_amd import device as dev
    a, b = on_device(c)
    return dev.smooth_values(b["x_trj"], b["u_trj"], a["dx"], a["du"], a["fz"], a["f0"], b["fnom"])


def assert_affine(o, ref, rows=None):
    for key, want in zip(("At", "Bt", "ct"), ref):
        got = o[key].cpu().numpy()
        if rows is not None:
            got, want = got[rows], want[rows]
        np.testing.assert_allclose(got, want, err_msg=key, **TOL_AB)


# ---------------------------------------------------------------- the kernel against the f64 statement
@pytest.mark.parametrize("T", vc.HORIZONS)
@pytest.mark.parametrize("n,m", vc.SIZES)
def test_values_pass_vs_numpy_statement(amd, n, m, T):
    from irs_mpc_amd import device as dev
    for N in vc.sample_counts(n, m):
        c = vc.make_case(n, m, T, N)
        geo = dev.smooth_values_geometry(T, N)
        assert geo["nblk"] == -(-N // 256)                   # T <= 3: one workgroup per 256 samples
        if N == 1000:
            assert geo["nblk"] == 4 and geo["chunk"] == 256 and N % geo["chunk"] == 232     # ragged last workgroup
        o = run_fused(c)
        assert (o["info"].cpu().numpy() == 0).all(), (N, o["info"])
        assert_affine(o, vc.reference(c))
        sums, scale = vc.sums_reference(c)
        err = np.abs(o["sums"].cpu().numpy() - sums)
        assert (err <= SUMS_BOUND * scale).all(), (N, float((err / scale).max()))
        o2 = run_fused(c)
        for key in ("sums", "At", "Bt", "ct"):
            assert torch.equal(o[key], o2[key]), (N, key)


def test_shards_add(amd):
    from irs_mpc_amd import device as dev
    n, m, T, N, N1 = 13, 4, 3, 1000, 333
    c = vc.make_case(n, m, T, N)
    a, b = on_device(c)
    parts = []
    for lo, hi in ((0, N1), (N1, N)):
        parts.append(dev.smooth_values_accumulate(a["dx"][:, lo:hi].contiguous(), a["du"][:, lo:hi].contiguous(),
                                                  a["fz"][:, lo:hi].contiguous(), a["f0"]).clone())
    sums = parts[0] + parts[1]
    At, Bt, ct, info = dev.smooth_values_finalize(N, b["x_trj"], b["u_trj"], b["fnom"], sums)
    assert (info.cpu().numpy() == 0).all()
    assert_affine(dict(At=At, Bt=Bt, ct=ct), vc.reference(c))
    ref, scale = vc.sums_reference(c)
    assert (np.abs(sums.cpu().numpy() - ref) <= SUMS_BOUND * scale).all()
    # accumulate alone and the fused call hold the same statistics, bit for bit
    whole = dev.smooth_values_accumulate(a["dx"], a["du"], a["fz"], a["f0"])
    assert torch.equal(whole, run_fused(c)["sums"])


def test_default_workspace_is_per_stream(amd):
    """A workspace takes one call in flight: the wrappers' cached scratch is one buffer per (device, stream)."""
    from irs_mpc_amd import device as dev
    c = vc.make_case(5, 2, 3, 1000)
    ref = vc.reference(c)
    a, b = on_device(c)
    torch.cuda.synchronize()
    outs, bufs = [], []
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(s):
            bufs.append(dev._values_workspace(5, 2, 3, 1000, a["dx"].device))
            outs.append(dev.smooth_values(b["x_trj"], b["u_trj"], a["dx"], a["du"], a["fz"], a["f0"], b["fnom"]))
    torch.cuda.synchronize()
    assert bufs[0].data_ptr() != bufs[1].data_ptr()
    for o in outs:
        assert_affine(o, ref)
    assert torch.equal(outs[0]["sums"], outs[1]["sums"])


@pytest.mark.parametrize("n,m", [(5, 2), (32, 16)])
def test_rank_deficient(amd, n, m):
    d = n + m
    o = run_fused(vc.make_case(n, m, 3, d - 1))
    assert (o["info"].cpu().numpy() > 0).all(), o["info"]
    assert (o["info"].cpu().numpy() <= d).all(), o["info"]


@pytest.mark.parametrize("n,m", [(5, 2), (17, 1)])
def test_non_finite_value_marks_its_timestep_only(amd, n, m):
    d = n + m
    c = vc.make_case(n, m, 3, 4 * d + 1)
    ref = vc.reference(c)                                    # of the finite inputs: rows 0 and 2 are unchanged
    c["fz"] = c["fz"].copy()
    c["fz"][1, 7, n - 1] = np.inf
    o = run_fused(c)
    assert o["info"].cpu().numpy().tolist() == [0, d + 1, 0]
    assert_affine(o, ref, rows=[0, 2])


def test_element_offsets_beyond_2_to_31(amd):
    """A (1, N, 16) du of more than 2^31 floats (8.6 GB; no tensor that crosses 2^31 elements is smaller -- dx and fz,
    one column each, add 0.5 GB apiece): all zeros (exact zeros in every statistic) except the last 1000 samples, which
    start at du's element 2^31 and hold a small case -- the pass must find exactly that case there.  All three tensors
    go through the same span loader with the same 64-bit element offsets."""
    from irs_mpc_amd import device as dev
    n, m, tail = 1, 16, 1000
    N = 2 ** 27 + tail
    c = vc.make_case(n, m, 1, tail)
    a, b = on_device(c)
    big = {k: torch.zeros((1, N, a[k].shape[2]), dtype=dev.F32, device="cuda") for k in ("dx", "du", "fz")}
    for k in big:
        big[k][:, N - tail:] = a[k]
    big["fz"][:, :N - tail] = a["f0"][:, None, :]            # dF = fz - f0 = 0 on the padding samples
    geo = dev.smooth_values_geometry(1, N)                   # the cap of 4096 workgroups: 32 769 samples each, rounded
    assert (geo["chunk"], geo["nblk"]) == (33024, 4065)      # up to whole 256-thread trips
    o = dev.smooth_values(b["x_trj"], b["u_trj"], big["dx"], big["du"], big["fz"], a["f0"], b["fnom"])
    assert int(o["info"].item()) == 0
    assert_affine(o, vc.reference(c))
    sums, scale = vc.sums_reference(c)
    assert (np.abs(o["sums"].cpu().numpy() - sums) <= SUMS_BOUND * scale).all()
    del big
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- torch-defined systems
class TorchPendulum(pkg.TorchDynamicalSystem):
    """oracle.PendulumOracle.dynamics_batch in torch."""

    def __init__(self, h):
        super().__init__()
        self.h, self.dim_x, self.dim_u = h, 2, 1

    def dynamics_batch_torch(self, x, u):
        angle, speed, torque = x[:, 0], x[:, 1], u[:, 0]
        next_speed = speed + self.h * (-torch.sin(angle) + torque)
        next_angle = angle + self.h * next_speed
        return torch.stack([next_angle, next_speed], dim=1)


MC, MP, LEN, GRAV = 1.0, 0.1, 0.5, 9.81


class TorchCartPole(pkg.TorchDynamicalSystem):
    """Cart-pole, explicit Euler; x = (position, angle from the downward vertical, their rates), u = force on the cart.
    No device functor has this model."""

    def __init__(self, h):
        super().__init__()
        self.h, self.dim_x, self.dim_u = h, 4, 1

    def dynamics_batch_torch(self, x, u):
        th, xd, thd, f = x[:, 1], x[:, 2], x[:, 3], u[:, 0]
        s, c = torch.sin(th), torch.cos(th)
        den = MC + MP * s * s
        xdd = (f + MP * s * (LEN * thd * thd + GRAV * c)) / den
        thdd = (-f * c - MP * LEN * thd * thd * c * s - (MC + MP) * GRAV * s) / (LEN * den)
        return x + self.h * torch.stack([xd, thd, xdd, thdd], dim=1)


class NumpyCartPole:
    """The same model with the oracle's system interface."""

    def __init__(self, h):
        self.h, self.dim_x, self.dim_u = h, 4, 1

    def dynamics_batch(self, x, u):
        th, xd, thd, f = x[:, 1], x[:, 2], x[:, 3], u[:, 0]
        s, c = np.sin(th), np.cos(th)
        den = MC + MP * s * s
        xdd = (f + MP * s * (LEN * thd * thd + GRAV * c)) / den
        thdd = (-f * c - MP * LEN * thd * thd * c * s - (MC + MP) * GRAV * s) / (LEN * den)
        return x + self.h * np.stack([xd, thd, xdd, thdd], axis=1)

    def dynamics(self, x, u):
        return self.dynamics_batch(np.asarray(x, float)[None, :], np.asarray(u, float)[None, :])[0]


def pend_params(T):
    p = pkg.IrsLqrParameters()
    p.Q, p.Qd, p.R = np.diag([1., 1.]), np.diag([20., 20.]), np.diag([1.])
    p.x0 = np.array([0., 0.])
    p.xd_trj = np.tile(np.array([np.pi, 0.]), (T + 1, 1))
    p.u_trj_initial = np.tile(np.array([0.1]), (T, 1))
    p.xbound = [-np.array([1e4, 1e4]), np.array([1e4, 1e4])]
    p.ubound = np.array([-np.array([1e4]), np.array([1e4])])        # finite, never binding: the plan test runs
    return p


def cartpole_params(T):
    p = pkg.IrsLqrParameters()
    p.Q, p.Qd, p.R = np.diag([1., 5., 0.1, 0.1]), np.diag([10., 50., 1., 1.]), np.diag([0.1])
    p.x0 = np.array([0., 0.3, 0., 0.])
    p.xd_trj = np.tile(np.array([0.5, np.pi, 0., 0.]), (T + 1, 1))
    p.u_trj_initial = np.tile(np.array([0.2]), (T, 1))
    return p


class Replay:
    """sampling closure that replays recorded draws (one (N,n),(N,m) pair per call)."""

    def __init__(self, dx, du):
        self.dx, self.du, self.i = dx, du, 0

    def __call__(self, x, u, it):
        i = self.i % len(self.dx)
        self.i += 1
        return self.dx[i], self.du[i]


def assert_tv(got, want):
    for g, w, key in zip(got, want, ("At", "Bt", "ct")):
        np.testing.assert_allclose(g, w, err_msg=key, **TOL_AB)


def test_torch_pendulum_matches_the_compiled_functor(amd):
    T, N = 30, 257
    rng = np.random.default_rng(5)
    dx = rng.normal(size=(T, N, 2)).astype(np.float32)
    du = rng.normal(size=(T, N, 1)).astype(np.float32)
    sol_t = amd.IrsLqrZeroOrder(TorchPendulum(0.05), pend_params(T), Replay(dx, du))
    sol_c = amd.IrsLqrZeroOrder(amd.PendulumDynamics(0.05), pend_params(T), Replay(dx, du))
    np.testing.assert_allclose(sol_t.x_trj, sol_c.x_trj, rtol=0, atol=1e-12)
    assert abs(sol_t.cost - sol_c.cost) <= 1e-12 * abs(sol_c.cost)
    assert_tv(sol_t.get_TV_matrices(sol_t.x_trj, sol_t.u_trj), sol_c.get_TV_matrices(sol_c.x_trj, sol_c.u_trj))
    # the reference's four virtuals are served from the callable
    X, U = rng.normal(size=(9, 2)), rng.normal(size=(9, 1))
    s_t, s_o = TorchPendulum(0.05), orc.PendulumOracle(0.05)
    np.testing.assert_allclose(s_t.dynamics_batch(X, U), s_o.dynamics_batch(X, U), rtol=0, atol=1e-14)
    np.testing.assert_allclose(s_t.dynamics(X[0], U[0]), s_o.dynamics(X[0], U[0]), rtol=0, atol=1e-14)
    np.testing.assert_allclose(s_t.jacobian_xu_batch(X, U), s_o.jacobian_xu_batch(X, U), rtol=0, atol=1e-14)
    np.testing.assert_allclose(s_t.jacobian_xu(X[0], U[0]), s_o.jacobian_xu(X[0], U[0]), rtol=0, atol=1e-14)


@pytest.mark.parametrize("fix,cls", [("pendulum_zero_T30_N100", "IrsLqrZeroOrder"),
                                     ("pendulum_first_T30_N100", "IrsLqrFirstOrder")])
def test_torch_pendulum_reproduces_the_reference_fixtures(amd, golden_dir, fix, cls):
    f = np.load(os.path.join(golden_dir, fix + ".npz"))
    sol = getattr(amd, cls)(TorchPendulum(float(f["h"])), pend_params(30), Replay(f["dx"], f["du"]))
    assert_tv(sol.get_TV_matrices(sol.x_trj, sol.u_trj), (f["At"], f["Bt"], f["ct"]))


def test_torch_pendulum_exact_reproduces_the_reference_csv(amd, golden_dir):
    gold = np.loadtxt(os.path.join(golden_dir, "pendulum_exact.csv"))[:3]
    sol = amd.IrsLqrExact(TorchPendulum(0.05), pend_params(200))
    sol.verbose = False                                      # a compiled system would take the fused loop here
    assert sol._fused_spec() is None
    sol.iterate(1)
    np.testing.assert_allclose(sol.cost_lst, gold, rtol=2e-9)


@pytest.fixture(scope="module")
def cartpole_case():
    T, N = 12, 400
    rng = np.random.default_rng(11)
    dx = (0.1 * rng.normal(size=(T, N, 4))).astype(np.float32)
    du = (0.1 * rng.normal(size=(T, N, 1))).astype(np.float32)
    return T, N, dx, du


def test_system_without_a_functor_zero_order_and_descent(amd, cartpole_case):
    T, N, dx, du = cartpole_case
    p, s_o = cartpole_params(T), NumpyCartPole(0.02)
    sol = amd.IrsLqrZeroOrder(TorchCartPole(0.02), p, Replay(dx, du))
    np.testing.assert_allclose(sol.x_trj, orc.rollout(s_o, p.x0, p.u_trj_initial), rtol=0, atol=1e-12)
    got = sol.get_TV_matrices(sol.x_trj, sol.u_trj)
    assert_tv(got, orc.zero_order_TV(s_o, sol.x_trj, sol.u_trj, dx.astype(np.float64), du.astype(np.float64)))
    # Riccati + closed-loop rollout through the callable, against the oracle on the device's own linearisation
    x_new, u_new = sol.local_descent(sol.x_trj, sol.u_trj)
    At, Bt, ct = (sol._last[k].cpu().numpy() for k in ("At", "Bt", "ct"))
    xo, uo, _, _ = orc.local_descent(s_o, At, Bt, ct, p.Q, p.Qd, p.R, p.x0, p.xd_trj)
    np.testing.assert_allclose(x_new, xo, rtol=0, atol=1e-8)
    np.testing.assert_allclose(u_new, uo, rtol=0, atol=1e-8)


@pytest.mark.parametrize("n,m", [(4, 1), (12, 4), (32, 16), (1, 1)])
def test_any_size_device_rng_matches_specification(amd, n, m):
    """irs_values_rng_samples against the stream's f64 statement at the tolerance irs_rng_samples is held to
    (tests/test_gpu_parity.py::test_device_rng_matches_specification: rtol 2e-5, atol 2e-6), plus, for the pairs whose
    u1 lies within 2^-6 of 1 (radius sqrt(-2 ln u1) < 0.177), the stream's documented loss there (csrc/philox.hpp,
    irs_hip.h at irs_cem_candidates): u1 = (r + 0.5) / 2^32 is formed in f32, two roundings of 2^-24 relative each, so
    -2 ln u1 is off by up to 2 * 2^-23 / u1 and the radius by up to 2^-23 / (u1 rad) <= 2^-22 / rad -- at most
    sqrt(2 * 2^-23) = 4.9e-4 where u1 rounds to 1 -- times the component's std.  (The 48 000 draws of the compiled
    stream's own test hold no such pair; the 144 000 of the largest size here hold one.)"""
    from irs_mpc_amd import _lib, device as dev
    lib, T, N, seed, it, off = _lib.load(), 3, 1000, 0x123456789ABC, 4, 77
    std_x, std_u = 0.1 * np.arange(1, n + 1), 0.2 * np.arange(1, m + 1)

    def draw(fn, N, off):
        dx = torch.empty((T, N, n), dtype=dev.F32, device="cuda")
        du = torch.empty((T, N, m), dtype=dev.F32, device="cuda")
        _lib.check(fn(n, m, T, N, _lib.dbl_array(std_x), _lib.dbl_array(std_u), seed, it, off, dx.data_ptr(),
                      du.data_ptr(), dev._stream()), "rng samples")
        return dx, du

    dx, du = draw(lib.irs_values_rng_samples, N, off)
    # the statement, drawn with m padded to whole Philox blocks (unit std) so that every component's Box-Muller partner,
    # and with it the pair's radius, is at hand; components < n + m are the (n, m) stream's
    d, pad = n + m, -(n + m) % 4
    ox, ou = orc.device_gaussian_samples(T, N, n, m + pad, std_x, np.concatenate([std_u, np.ones(pad)]), seed, it,
                                         sample_offset=off)
    want = np.concatenate([ox, ou], axis=2)
    std = np.concatenate([std_x, std_u, np.ones(pad)])
    unit = want / std
    rad = np.repeat(np.hypot(unit[:, :, 0::2], unit[:, :, 1::2]), 2, axis=2)
    tol = 2e-5 * np.abs(want) + 2e-6
    near_one = rad < 0.177
    tol[near_one] += np.minimum(std * 2.0 ** -22 / np.maximum(rad, 1e-300), std * 4.9e-4)[near_one]
    got = np.concatenate([dx.cpu().numpy(), du.cpu().numpy()], axis=2)
    assert (np.abs(got - want[:, :, :d]) <= tol[:, :, :d]).all()
    dx2, du2 = draw(lib.irs_values_rng_samples, 400, off + 600)        # the split over devices keeps the stream
    assert torch.equal(dx2, dx[:, 600:]) and torch.equal(du2, du[:, 600:])


def test_system_without_a_functor_device_drawn_samples(amd, cartpole_case):
    T, N, _, _ = cartpole_case
    p = cartpole_params(T)
    std_x, std_u, seed = [0.1, 0.1, 0.2, 0.2], [0.3], 3
    sm = amd.GaussianSmoothing(std_x, std_u, N, seed=seed)
    sol_g = amd.IrsLqrZeroOrder(TorchCartPole(0.02), p, sm)
    assert sol_g._fused_spec() is None                       # never the fused irs_iterate loop
    dxo, duo = orc.device_gaussian_samples(T, N, 4, 1, std_x, std_u, seed, 1, dtype=np.float32)
    sol_r = amd.IrsLqrZeroOrder(TorchCartPole(0.02), p, Replay(dxo, duo))
    assert_tv(sol_g.get_TV_matrices(sol_g.x_trj, sol_g.u_trj), sol_r.get_TV_matrices(sol_r.x_trj, sol_r.u_trj))
    # the shard entries: two halves of the stream, offset, add up to the whole
    dm = sol_g._dm
    from irs_mpc_amd import device as dev
    from irs_mpc_amd._lib import SMOOTH_ZERO_ORDER_AB
    x, u = dev.to_dev(sol_g.x_trj), dev.to_dev(sol_g.u_trj)
    sx, su = sm.stds(1)
    s0 = dm.smooth_accumulate_rng(SMOOTH_ZERO_ORDER_AB, x, u, 150, sx, su, seed, 1, sample_offset=0).clone()
    s1 = dm.smooth_accumulate_rng(SMOOTH_ZERO_ORDER_AB, x, u, N - 150, sx, su, seed, 1, sample_offset=150)
    At, Bt, ct, info = dm.smooth_finalize(SMOOTH_ZERO_ORDER_AB, N, x, u, s0 + s1)
    assert (info.cpu().numpy() == 0).all()
    assert_tv((At.cpu().numpy(), Bt.cpu().numpy(), ct.cpu().numpy()), sol_r.get_TV_matrices(sol_r.x_trj, sol_r.u_trj))
    # a quiet run goes descent by descent through the callable
    sol_g.verbose = False
    sol_g.iterate(1)
    assert len(sol_g.cost_lst) == 3 and np.isfinite(sol_g.cost_lst).all()


def test_bounds_that_bind_need_a_compiled_model(amd):
    T, N = 30, 100
    rng = np.random.default_rng(2)
    dx = rng.normal(size=(T, N, 2)).astype(np.float32)
    du = rng.normal(size=(T, N, 1)).astype(np.float32)
    p = pend_params(T)                                       # |u| <= 1e4: finite, never active
    sol = amd.IrsLqrZeroOrder(TorchPendulum(0.05), p, Replay(dx, du))
    x_new, u_new = sol.local_descent(sol.x_trj, sol.u_trj)
    assert np.abs(u_new).max() > 0.05 and sol._box_bounds() is not None
    p = pend_params(T)
    p.ubound = np.array([[-0.05], [0.05]])                   # the unconstrained plan leaves this box
    sol = amd.IrsLqrZeroOrder(TorchPendulum(0.05), p, Replay(dx, du))
    with pytest.raises(NotImplementedError, match="compiled"):
        sol.local_descent(sol.x_trj, sol.u_trj)
