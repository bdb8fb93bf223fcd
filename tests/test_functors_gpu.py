"""The tables of tests/helpers/functor_reference.py through the compiled library, per sample.

tests/test_functors_cpu.py admits reference and bounds on a host build of csrc/dual.hpp and csrc/models.hpp; the device
objects are built with other flags (-ffp-contract=fast everywhere, -ffinite-math-only -fno-signed-zeros on the sample
pass), so the same tables go through the library here:
  f64   dynamics_batch, jacobian_xu_batch and the scalar forms -- step<double> and the Dual<double> Jacobian;
  f32   one launch of the sample pass per model and mode with N = 1 and T = the table length: timestep t has the nominal
        point xb = xs - z and the single sample z = +-2^-6 in every component (xb, xs exact in f32), so the z df' block
        of ZERO_ORDER_AB's sums divided by z is that sample's f32 df = step<float>(xs) - step<float>(xb) exactly as the
        kernel formed it, and FIRST_ORDER's sums are the sample's f32 Jacobian at xs -- the quadrotor's through step_jac
        and expand_entry, the others' through the duals;
  irs_sincos on the device: the pendulum with h = 1 has xn[1] = -sin(theta) and J[1][0] = -cos(theta) exactly;
  the extreme draws of tests/golden/rng_extremes.json from both generators (rng_samples, cem_candidates).
The batched general pass draws its samples on the device only (smooth_rng_general_batch): it has no supplied-sample
route, so it has no twin here.

Largest error / bound per model and regime, on an MI355X, as the tests print them (pytest -s).  Columns: step<double>
(dynamics_batch), Dual<double> Jacobian (jacobian_xu_batch), the f32 sample's step difference (ZERO_ORDER_AB), the f32
sample's Jacobian (FIRST_ORDER; quadrotor: step_jac + expand_entry).  No regime needs more than the counted K.
    pendulum    theta_1e-2     0.086 0.135 0.077 0.198
    pendulum    theta_1e-1     0.069 0.125 0.064 0.198
    pendulum    theta_1e0      0.068 0.142 0.046 0.198
    pendulum    theta_1e1      0.063 0.130 0.046 0.198
    pendulum    theta_1e2      0.055 0.132 0.055 0.198
    pendulum    k_pi_2         0.067 0.166 0.064 0.198
    quadrotor   moderate       0.040 0.099 0.024 0.182
    quadrotor   pitch_0.3      0.046 0.080 0.031 0.100
    quadrotor   pitch_0.1      0.046 0.129 0.022 0.063
    quadrotor   pitch_1e-2     0.041 0.290 0.019 0.168
    quadrotor   roll_yaw_1e3   0.031 0.185 0.026 0.086
    quadrotor   rates_0_large  0.117 0.170 0.048 0.115
    quadrotor   zero_thrust    0.030 0.132 0.028 0.107
    bicycle     moderate       0.073 0.083 0.068 0.097
    bicycle     steer_0.1      0.069 0.063 0.061 0.086
    bicycle     steer_1e-2     0.073 0.059 0.055 0.072
    bicycle     speed_0_neg    0.070 0.092 0.061 0.081
    bicycle     heading_1e3    0.072 0.074 0.066 0.105
    three_cart  stuck_123      0.062 0.045 0.035 0.045
    three_cart  contact_12 / contact_23 / free    0 (every operation exact on the dyadic rows)
    three_cart  surface        0.036 0.045 0.045 0.045
irs_sincos f64 on the device: 1.24 ulp over the sweep, 450.94 ulp at the f64 neighbours of k pi/2 (as on the host).
Extreme draws: the smoothing stream at most 0.68 of its tolerance (19.9 x the plain rtol 2e-5 / atol 2e-6 at the largest
u1 words: the documented tail), the candidate stream at most 0.21 of the plain tolerance.
"""
import numpy as np
import pytest
import torch

from oracle import smooth_cases as sc
from tests.helpers import functor_reference as fr

pytestmark = pytest.mark.gpu

MODEL_NAMES = list(fr.MODELS)


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()     # fails loudly if the HIP library is missing
    return irs_mpc_amd


_systems = {}


def system(amd, name, h=None):
    key = (name, h)
    if key not in _systems:
        M = fr.MODELS[name]
        s = getattr(amd, fr.SYSTEM_CLASSES[name][0])(M["params"][0] if h is None else h)
        if name == "three_cart":
            s.d = M["params"][1]
        assert h is not None or [float(p) for p in s.device_params()] == [float(p) for p in M["params"]], name
        _systems[key] = s
    return _systems[key]


def npy(t):
    return t.detach().cpu().numpy()


_tab = {}


def table(name):
    """(regime tags, row ranges, V = all rows [xs | us] f32, references at the rows) of a model, computed once."""
    if name not in _tab:
        T = fr.tables(name)
        n = fr.MODELS[name]["n"]
        V = np.concatenate(list(T.values()))
        spans, at = {}, 0
        for tag, v in T.items():
            spans[tag] = slice(at, at + v.shape[0])
            at += v.shape[0]
        _tab[name] = (spans, V, fr.references(name, V[:, :n], V[:, n:]))
    return _tab[name]


def ratios(name, spans, err, bnd, label):
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bnd)
    for tag, s in spans.items():
        print("%-10s %-14s %-22s max error / bound %.3f" % (name, tag, label, q[s].max()))
    return q


def errs(refs, got, what):
    return np.stack([fr.error(r, g, what) for r, g in zip(refs, got)])


def bounds(name, refs, prec, what):
    return np.stack([fr.bound(name, r, prec, what) for r in refs])


# ---------------------------------------------------------------------------------------------------------------- f64
@pytest.mark.parametrize("name", MODEL_NAMES)
def test_f64_step_and_jacobian_within_bounds(amd, name):
    """dynamics_batch / jacobian_xu_batch over every table, and the scalar forms on the first row of every regime (equal
    to the batch's row bit for bit)."""
    from irs_mpc_amd import device as dev
    spans, V, refs = table(name)
    n = fr.MODELS[name]["n"]
    s = system(amd, name)
    X, U = V[:, :n].astype(np.float64), V[:, n:].astype(np.float64)
    f = npy(s.dm().dynamics_batch(dev.to_dev(X), dev.to_dev(U)))
    J = npy(s.dm().jacobian_xu_batch(dev.to_dev(X), dev.to_dev(U)))
    assert np.isfinite(f).all() and np.isfinite(J).all()
    qf = ratios(name, spans, errs(refs, f, "f"), bounds(name, refs, "f64", "f"), "step<double>")
    qJ = ratios(name, spans, errs(refs, J, "J"), bounds(name, refs, "f64", "J"), "Dual<double> Jacobian")
    assert (qf <= 1.0).all() and (qJ <= 1.0).all()
    for sp in spans.values():
        i = sp.start
        np.testing.assert_array_equal(s.dynamics(X[i], U[i]), f[i])
        np.testing.assert_array_equal(s.jacobian_xu(X[i], U[i]), J[i])


# ------------------------------------------------------------------------------------------------- f32, per sample
MAX_T = 1024        # timesteps per launch of the sample pass (its arrival counters)


def accumulate(dm, mode, x_trj, u_trj, dx, du):
    """smooth_accumulate of numpy inputs with N = 1, in launches of at most MAX_T timesteps: sums (T, P) as numpy."""
    from irs_mpc_amd import device as dev
    out = []
    for a in range(0, x_trj.shape[0], MAX_T):
        r = slice(a, a + MAX_T)
        out.append(npy(dm.smooth_accumulate(mode, dev.to_dev(x_trj[r]), dev.to_dev(u_trj[r]),
                                            dev.to_dev(np.ascontiguousarray(dx[r]), dev.F32),
                                            dev.to_dev(np.ascontiguousarray(du[r]), dev.F32))))
    return np.concatenate(out)


def sample_pass(amd, name, mode):
    """The N = 1 launch described in the module docstring: (sums (T, P), z (T, d), xb, ub f64)."""
    from irs_mpc_amd import device as dev
    _, V, _ = table(name)
    n = fr.MODELS[name]["n"]
    z = fr.sample_of(V)
    Vb = (V - z).astype(np.float32)
    assert np.array_equal(Vb.astype(np.float64) + z, V.astype(np.float64))
    xb, ub = Vb[:, :n].astype(np.float64), Vb[:, n:].astype(np.float64)
    dm = system(amd, name).dm()
    sums = accumulate(dm, mode, xb, ub, z[:, None, :n], z[:, None, n:])
    return sums, z.astype(np.float64), xb, ub


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_f32_sample_step_difference_within_bounds(amd, name):
    """ZERO_ORDER_AB, N = 1: every row z_i df' / z_i of the sums is the same f32 df, bit for bit, and it is within
    bound(xs) + bound(xb) + 2^-24 (|df| + both bounds) -- one rounding of the difference -- of the reference's
    f(xs) - f(xb)."""
    spans, V, refs = table(name)
    M = fr.MODELS[name]
    n, m = M["n"], M["m"]
    sums, z, xb, ub = sample_pass(amd, name, sc.ZERO_ORDER_AB)
    lay = sc.sums_layout(n, m, sc.ZERO_ORDER_AB, False)
    assert sums.shape[1] == lay["zdf"].stop
    zdf = sums[:, lay["zdf"]].reshape(-1, n + m, n)
    df = zdf / z[:, :, None]
    assert np.isfinite(df).all()
    assert (df == df[:, :1]).all(), "the rows of z df' disagree"
    gram = sums[:, lay["gram"]]
    assert (np.abs(gram) == fr.Z_MAG ** 2).all()
    df = df[:, 0]
    refs_b = fr.references(name, xb, ub, jac=False)
    want_hi = fr.stack(refs, "f_hi") - fr.stack(refs_b, "f_hi")
    want_lo = fr.stack(refs, "f_lo") - fr.stack(refs_b, "f_lo")
    err = np.abs((df - want_hi) - want_lo)
    b2 = bounds(name, refs, "f32", "f") + bounds(name, refs_b, "f32", "f")
    bnd = b2 + fr.EPS["f32"] * (np.abs(want_hi) + b2)
    q = ratios(name, spans, err, bnd, "step<float> difference")
    assert (q <= 1.0).all()


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_f32_sample_jacobian_within_bounds(amd, name):
    """FIRST_ORDER, N = 1: the sums are the sample's f32 Jacobian at (xs, us); smooth_finalize hands the same numbers
    back as [At | Bt].  The three-cart rows on a switching surface and one f32 step to either side carry the Jacobian of
    the branch strict `<` gives (the branches differ by at least 1/6 in some entry; allowed: the rounding of 1/3)."""
    from irs_mpc_amd import device as dev
    spans, V, refs = table(name)
    M = fr.MODELS[name]
    n, m = M["n"], M["m"]
    d = n + m
    sums, z, xb, ub = sample_pass(amd, name, sc.FIRST_ORDER)
    assert sums.shape[1] == n * d
    J = sums.reshape(-1, n, d)
    assert np.isfinite(J).all()
    q = ratios(name, spans, errs(refs, J, "J"), bounds(name, refs, "f32", "J"), "f32 sample Jacobian")
    assert (q <= 1.0).all()
    dm = system(amd, name).dm()
    At, Bt, _, info = dm.smooth_finalize(sc.FIRST_ORDER, 1, dev.to_dev(xb), dev.to_dev(ub), dev.to_dev(sums))
    assert not npy(info).any()
    np.testing.assert_array_equal(np.concatenate([npy(At), npy(Bt)], axis=2), J)
    if name == "three_cart":
        s = spans["surface"]
        assert (np.abs(J[s] - fr.stack(refs, "J_hi")[s]) <= 2.0 ** -24).all()


# -------------------------------------------------------------------------------------------- irs_sincos on the device
def test_irs_sincos_f64_on_the_device(amd):
    """Pendulum, h = 1, speed 0, torque 0: xn[1] = -sin(theta) and J[1][0] = -cos(theta) with no rounding of their own.
    The bounds of tests/test_functors_cpu.py: 2 ulp over the sweep, 564 ulp of the tiny member of the pair at the f64
    neighbours of k pi/4 (1.25 x the 450.94 ulp measured on the host against mpmath)."""
    from irs_mpc_amd import device as dev
    _, x64, near = fr.sincos_points()
    s = system(amd, "pendulum", h=1.0)
    X = np.column_stack([x64, np.zeros_like(x64)])
    U = np.zeros((x64.size, 1))
    f = npy(s.dm().dynamics_batch(dev.to_dev(X), dev.to_dev(U)))
    J = npy(s.dm().jacobian_xu_batch(dev.to_dev(X), dev.to_dev(U)))
    got = np.column_stack([-f[:, 1], -J[:, 1, 0]])
    hi, lo = fr.sincos_reference(x64)
    q = np.abs((got - hi) - lo) / np.spacing(np.abs(hi))
    print("device irs_sincos f64: sweep and edges %.3f ulp, neighbours of k pi/4 %.3f ulp" % (q[~near].max(), q[near].max()))
    assert np.isfinite(got).all()
    assert (q[~near] <= fr.SINCOS_ULP_F64).all()
    assert (q[near] <= fr.SINCOS_ULP_F64_NEIGHBOURS).all()


def test_irs_sincos_f32_on_the_device(amd):
    """Pendulum, h = 1, one timestep per point.  FIRST_ORDER with the sample z = 0: the sums' J[1][0] = -cos(x) in f32,
    held to 1.5e-7.  ZERO_ORDER_AB from the nominal point 0 with the sample (x, 0, 1): df[1] = fl(1 - sin x), read from
    the torque's row of z df' (z = 1), held to 1.5e-7 + 2^-24 for that one rounding below 2."""
    from irs_mpc_amd import device as dev
    x32, _, _ = fr.sincos_points()
    T = x32.size
    dm = system(amd, "pendulum", h=1.0).dm()
    hi, lo = fr.sincos_reference(x32)
    xt = np.column_stack([x32.astype(np.float64), np.zeros(T)])
    J = accumulate(dm, sc.FIRST_ORDER, xt, np.zeros((T, 1)), np.zeros((T, 1, 2), np.float32),
                   np.zeros((T, 1, 1), np.float32)).reshape(T, 2, 3)
    err_c = np.abs((-J[:, 1, 0] - hi[:, 1]) - lo[:, 1])
    dx = np.zeros((T, 1, 2), np.float32)
    dx[:, 0, 0] = x32
    sums = accumulate(dm, sc.ZERO_ORDER_AB, np.zeros((T, 2)), np.zeros((T, 1)), dx, np.ones((T, 1, 1), np.float32))
    lay = sc.sums_layout(2, 1, sc.ZERO_ORDER_AB, False)
    df1 = sums[:, lay["zdf"]].reshape(T, 3, 2)[:, 2, 1]
    err_s = np.abs(((1.0 - df1) - hi[:, 0]) - lo[:, 0])
    print("device irs_sincos f32: max |error| cos %.3e, sin (through 1 - sin) %.3e" % (err_c.max(), err_s.max()))
    assert np.isfinite(J).all() and np.isfinite(sums).all()
    assert (err_c <= fr.SINCOS_ABS_F32).all()
    assert (err_s <= fr.SINCOS_ABS_F32 + 2.0 ** -24).all()


# --------------------------------------------------------------------------------------------------------------- RNG
def _extreme_draws(fetch):
    g = fr.rng_extremes()
    idx = fr.rng_extreme_indices(g)
    z, rad = fr.box_muller(fr.philox_words(idx))
    got = np.stack([fetch(i) for i in idx])
    return g, idx, z, rad, got


def test_smoothing_stream_extreme_draws(amd):
    """rng_samples(T = 1, N = 1, sample_offset = index) at the committed extremes -- the smallest and largest u1 words of
    2^24 draws, u2 next to every quadrant boundary and rintf tie -- against the mpmath Box-Muller: rtol 2e-5 / atol 2e-6
    plus the radius deviation of forming u1 in f32, min(rad, 2^-25 / rad (1 + 2^-20))."""
    dm = system(amd, "quadrotor").dm()
    ones_x, ones_u = np.ones(12), np.ones(4)

    def fetch(i):
        return npy(dm.rng_samples(1, 1, ones_x, ones_u, fr.RNG_SEED, fr.RNG_IT, sample_offset=i)[0])[0, 0, :4]
    g, idx, z, rad, got = _extreme_draws(fetch)
    err, tol = np.abs(got - z), fr.rng_tolerance(z, rad, exact_tail=False)
    print("smoothing stream: max |err| / tol = %.3f; against the plain tolerance %.3f"
          % ((err / tol).max(), (err / fr.rng_tolerance(z, rad, True)).max()))
    assert np.isfinite(got).all()
    assert (err <= tol).all()


def test_candidate_stream_extreme_draws(amd):
    """cem_candidates at the same extremes (mean 0, std 1, T = 1, m = 4, B = 1): the element-wise tolerance of
    test_candidate_stream_matches_specification, std (2e-5 |z| + 2e-6), with no deviation term -- the tail
    (philox_normal4<true>) that test was written for and never reaches."""
    from irs_mpc_amd import device as dev
    dm = system(amd, "pendulum").dm()
    mean, std = dev.to_dev(np.zeros((1, 4))), dev.to_dev(np.ones((1, 4)))

    def fetch(i):
        return npy(dm.cem_candidates(mean, std, 1, fr.RNG_SEED, fr.RNG_IT, sample_offset=i))[0, 0]
    g, idx, z, rad, got = _extreme_draws(fetch)
    err, tol = np.abs(got - z), fr.rng_tolerance(z, rad, exact_tail=True)
    print("candidate stream: max |err| / tol = %.3f" % (err / tol).max())
    assert np.isfinite(got).all()
    assert (err <= tol).all()
