"""The bounded TV-LQR problems on which the any-size kernel (csrc/boxqp_values.hip) is certified: sizes with no
compiled kernel, built exactly as oracle/boxqp_cases.py builds the compiled sizes' cases -- the same rng words
[n, m, T, 0, seed], hp.weights(..., "spd"), the sign flip, and its bound shapes B1 / B2 / B3 / B5 / B5u / B5x (plain
form only).  A case is a dict with that module's keys, so its statement / solve / kkt / active / mutated_rows / pick_rho
serve these cases unchanged; nothing of that module or its tables is altered.

Sizes: both ends of 1 <= n <= 32, 1 <= m <= 16 and both sides of 16: (1,1), (3,2), (9,5), (17,9), (32,16), (32,1),
(1,16).  T = 12 wraps the kernel's 3-slot record ring four times; (1,1) also runs T = 1 (B5u, B5x) and T = 2 (B5).

Also here: a NumPy twin of examples/torch_systems.TorchCartPole and a LinearSystem whose dynamics is A_t x + B_t u + c_t
(the plant of the resumed-tails test), both with the oracle's system interface.
"""
import functools

import numpy as np

from oracle import boxqp_cases as bc
from oracle import tvlqr_highprec as hp

SIZES = [(1, 1), (3, 2), (9, 5), (17, 9), (32, 16), (32, 1), (1, 16)]
T_MAIN = 12
RELAX = bc.RELAX


def size_id(n, m):
    return "s%dx%d" % (n, m)


def _case_list():
    out = []
    for n, m in SIZES:
        out += [(n, m, s, T_MAIN) for s in ("B1", "B2", "B3")]
        if (n, m) == (1, 1):
            out += [(n, m, "B5u", 1), (n, m, "B5x", 1), (n, m, "B5", 2)]
    return out


CASES = {"%s-%s" % (size_id(n, m), shape): (n, m, shape, T) for n, m, shape, T in _case_list()}

# case id -> last word of the data's seed where it is not 0: the first one at which the case is admitted -- every kind
# of bound the shape declares binds, and every applicable mutation moves the solution (tests/test_box_values_cpu.py
# holds each case to that).  s9x5-B3 and s1x16-B2: a declared kind does not bind at word 0; s9x5-B1: at words 0 .. 2
# the tube is active at step 0 alone, which neither shift+ nor row0 changes
SEED = {"s9x5-B1": 3, "s9x5-B3": 1, "s1x16-B2": 1}

# the value of bc.RHOS with the fewest oracle iterations (bc.pick_rho; checked by tests/test_box_values_cpu.py)
RHO = {
    "s1x1-B1": 1.0, "s1x1-B2": 1.0, "s1x1-B3": 1.0, "s1x1-B5u": 10.0, "s1x1-B5x": 10.0, "s1x1-B5": 10.0,
    "s3x2-B1": 1.0, "s3x2-B2": 10.0, "s3x2-B3": 1.0,
    "s9x5-B1": 10.0, "s9x5-B2": 10.0, "s9x5-B3": 1.0,
    "s17x9-B1": 10.0, "s17x9-B2": 10.0, "s17x9-B3": 1.0,
    "s32x16-B1": 10.0, "s32x16-B2": 10.0, "s32x16-B3": 10.0,
    "s32x1-B1": 100.0, "s32x1-B2": 100.0, "s32x1-B3": 100.0,
    "s1x16-B1": 1.0, "s1x16-B2": 1.0, "s1x16-B3": 1.0,
}


@functools.lru_cache(maxsize=None)
def problem(n, m, T, seed):
    """bc.problem for a free size: A_t = I + 0.1 N(0,1), B_t and xd_t standard normal, c_t = 0.1 N(0,1), dense SPD
    weights on the 2^-30 grid; the sign of (x0, xd, c) chosen so that the unconstrained u[:, 0] peaks on the positive
    side.  Holds the unconstrained optimum (xs, us) from the extended-precision Riccati reference."""
    rng = np.random.default_rng([n, m, T, 0, seed])
    p = dict(At=np.eye(n) + 0.1 * rng.normal(size=(T, n, n)), Bt=rng.normal(size=(T, n, m)),
             ct=0.1 * rng.normal(size=(T, n)), xd=rng.normal(size=(T + 1, n)), x0=rng.normal(size=n), idx=None)
    p["Q"], p["Qd"], p["R"] = hp.weights(rng, n, m, "spd")
    xs, us = hp.solve_tvlqr(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["x0"], p["xd"], alpha_R=0.5)
    xs, us = xs.astype(float), us.astype(float)
    if us[np.argmax(np.abs(us[:, 0])), 0] < 0:
        p["ct"], p["xd"], p["x0"], xs, us = -p["ct"], -p["xd"], -p["x0"], -xs, -us
    p["xs"], p["us"] = xs, us
    return p


def bound_rows(p, shape):
    """bc.bound_rows for the plain shapes, on problem data `p`: (rows, declared)."""
    xs, us = p["xs"], p["us"]
    T, n, m = p["At"].shape[0], p["At"].shape[1], p["Bt"].shape[2]
    inf = np.inf
    r = dict(x_lo=np.full((T + 1, n), -inf), x_hi=np.full((T + 1, n), inf), u_lo=np.full((T, m), -inf),
             u_hi=np.full((T, m), inf), du_lo=np.full((T, m), -inf), du_hi=np.full((T, m), inf))
    t = np.arange(T)
    declared = []

    def side(name, tt, j, v, level):
        key = name + ("_hi" if v > 0 else "_lo")
        r[key][tt, j] = level
        return [(key, tt, j)]

    def window(name, tt, j, v):
        r[name + "_lo"][tt, j], r[name + "_hi"][tt, j] = 0.5 * v - 0.05 * abs(v), 0.5 * v + 0.05 * abs(v)
        return [(name + "_lo", tt, j), (name + "_hi", tt, j)]

    if shape in ("B1", "B2"):
        r["u_hi"][:, 0] = 0.5 * np.abs(us[:, 0]).max() * (1.0 + 0.3 * np.sin(1.3 * t))
        declared.append([("u_hi", tt, 0) for tt in t])
    if shape == "B2":
        even = t[::2]
        r["u_lo"][even, m - 1] = bc._inside(us[:, m - 1], even, frac_lo=0.4)[0]
        late = np.arange(T // 2, T + 1)
        i = bc._state_component(p, late)
        r["x_lo"][late, i], r["x_hi"][late, i] = bc._inside(xs[:, i], late, frac_lo=0.3, frac_hi=0.2)
        declared += [[("u_lo", tt, m - 1) for tt in even], [("x_lo", tt, i) for tt in late],
                     [("x_hi", tt, i) for tt in late]]
    if shape == "B3":
        i = bc._state_component(p, [T])
        declared += [side("x", T, i, xs[T, i], 0.6 * xs[T, i]), side("u", 0, 0, us[0, 0], 0.5 * us[0, 0]),
                     window("u", T - 1, m - 1, us[T - 1, m - 1])]
    if shape in ("B5", "B5u", "B5x"):
        i = bc._state_component(p, [T])
        slack = lambda v: 10.0 * np.sign(v) * (1.0 + abs(v))
        if shape == "B5":
            declared += [window("u", 0, 0, us[0, 0]), side("x", T, i, xs[T, i], 0.5 * xs[T, i])]
        elif shape == "B5u":
            declared.append(side("u", 0, 0, us[0, 0], 0.5 * us[0, 0]))
            side("x", T, i, xs[T, i], slack(xs[T, i]))
        else:
            side("u", 0, 0, us[0, 0], slack(us[0, 0]))
            declared.append(side("x", T, i, xs[T, i], 0.5 * xs[T, i]))
    return r, declared


def build(n, m, shape, T, seed, rho=None, cid=None):
    c = dict(problem(n, m, T, seed))
    rows, declared = bound_rows(c, shape)
    c.update(rows, id=cid, size=size_id(n, m), shape=shape, T=T, rho=rho, declared=declared)
    return c


@functools.lru_cache(maxsize=None)
def case(cid):
    n, m, shape, T = CASES[cid]
    return build(n, m, shape, T, SEED.get(cid, 0), RHO[cid], cid)


@functools.lru_cache(maxsize=None)
def reference(cid):
    """(x, u, iterations) of the oracle's ADMM at the settings the device is run with (eps 1e-10, cap 40000)."""
    return bc.solve(case(cid))


def all_declared_bind(c, x, u):
    act, _ = bc.active(c, x, u)
    return all(any(act[k][t, j] for k, t, j in group) for group in c["declared"])


def constant_bounds(c):
    """The B2 bounds of a case made constant in time, one row per argument (constant_bounds of
    tests/test_boxqp_cases_gpu.py, plain form): on u, per component the tightest finite level of its rows; on x, half
    the unconstrained peak of the component that peaks highest (steps 1 .. T), on that side only.
    Returns (x_lo, x_hi, u_lo, u_hi)."""
    n = c["At"].shape[1]
    lo, hi = c["u_lo"], c["u_hi"]
    u_lo = np.where(np.isfinite(lo).any(axis=0), np.where(np.isfinite(lo), lo, -np.inf).max(axis=0), -np.inf)
    u_hi = np.where(np.isfinite(hi).any(axis=0), np.where(np.isfinite(hi), hi, np.inf).min(axis=0), np.inf)
    i = int(np.argmax(np.abs(c["xs"][1:]).max(axis=0)))
    v = c["xs"][1 + int(np.argmax(np.abs(c["xs"][1:, i]))), i]
    x_lo, x_hi = np.full(n, -np.inf), np.full(n, np.inf)
    (x_hi if v > 0 else x_lo)[i] = 0.5 * v
    return x_lo, x_hi, u_lo, u_hi


RESUMED = ("s9x5-B2", "s32x16-B2")      # the resumed-tails cases
QP = dict(rho=10.0, max_iter=20000, eps=1e-10)


@functools.lru_cache(maxsize=None)
def resumed_reference(cid):
    """(bounds, x_new, u_new, iterations per tail) of orc.local_descent_box on the case's constant bounds with the
    linear model itself as the plant."""
    from oracle import irs_oracle as orc
    c = case(cid)
    b = constant_bounds(c)
    with np.errstate(invalid="ignore"):
        xo, uo, iters = orc.local_descent_box(LinearSystem(c["At"], c["Bt"], c["ct"]), c["At"], c["Bt"], c["ct"], c["Q"],
                                              c["Qd"], c["R"], c["x0"], c["xd"], *b, **QP)
    return b, xo, uo, iters


# ------------------------------------------------------------------------------------------------ torch systems
def cartpole_setup():
    """The cart-pole problem of the values-pass test (T = 12, N = 400 replayed samples of std 0.1): dict(h, T, Q, Qd, R,
    x0, xd, u0, dx, du)."""
    T, N = 12, 400
    rng = np.random.default_rng(11)
    dx = (0.1 * rng.normal(size=(T, N, 4))).astype(np.float32)
    du = (0.1 * rng.normal(size=(T, N, 1))).astype(np.float32)
    return dict(h=0.02, T=T, Q=np.diag([1., 5., 0.1, 0.1]), Qd=np.diag([10., 50., 1., 1.]), R=np.diag([0.1]),
                x0=np.array([0., 0.3, 0., 0.]), xd=np.tile(np.array([0.5, np.pi, 0., 0.]), (T + 1, 1)),
                u0=np.tile(np.array([0.2]), (T, 1)), dx=dx, du=du)


CARTPOLE_VELOCITY = 2       # the bounded velocity: the cart's


@functools.lru_cache(maxsize=None)
def cartpole_bounds():
    """On the oracle's own zero-order linearisation of the replayed samples: the unbounded descent (xn, un) and the
    bounds built from it as test_three_cart_box_descent_vs_oracle builds its own -- |u| at 0.6 of the unbounded peak,
    one velocity at 0.7 of its unbounded peak.  Returns dict(xhi (4), uhi (1), xn, un, lin=(At, Bt, ct))."""
    from oracle import irs_oracle as orc
    s = cartpole_setup()
    so = NumpyCartPole(s["h"])
    x_trj = orc.rollout(so, s["x0"], s["u0"])
    At, Bt, ct = orc.zero_order_TV(so, x_trj, s["u0"], s["dx"].astype(np.float64), s["du"].astype(np.float64))
    xn, un, _, _ = orc.local_descent(so, At, Bt, ct, s["Q"], s["Qd"], s["R"], s["x0"], s["xd"])
    xhi, uhi = np.full(4, np.inf), np.array([0.6 * np.abs(un[:, 0]).max()])
    xhi[CARTPOLE_VELOCITY] = 0.7 * np.abs(xn[:, CARTPOLE_VELOCITY]).max()
    return dict(xhi=xhi, uhi=uhi, xn=xn, un=un, lin=(At, Bt, ct))


def cartpole_bounded_descent(At, Bt, ct):
    """orc.local_descent_box of the cart-pole problem under cartpole_bounds() on the linearisation given:
    (x_new, u_new, iterations per tail)."""
    from oracle import irs_oracle as orc
    s, b = cartpole_setup(), cartpole_bounds()
    return orc.local_descent_box(NumpyCartPole(s["h"]), At, Bt, ct, s["Q"], s["Qd"], s["R"], s["x0"], s["xd"], -b["xhi"],
                                 b["xhi"], -b["uhi"], b["uhi"], **QP)


# ------------------------------------------------------------------------------------------------ plants
MC, MP, LEN, GRAV = 1.0, 0.1, 0.5, 9.81


class NumpyCartPole:
    """examples/torch_systems.TorchCartPole (its default constants) with the oracle's system interface."""

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


class LinearSystem:
    """x+ = A_t x + B_t u + c_t, t counted by the calls: orc.local_descent_box steps its plant once per t, in order."""

    def __init__(self, At, Bt, ct):
        self.At, self.Bt, self.ct, self.t = At, Bt, ct, 0
        self.dim_x, self.dim_u = At.shape[1], Bt.shape[2]

    def dynamics(self, x, u):
        t = self.t
        self.t += 1
        return self.At[t] @ x + self.Bt[t] @ u + self.ct[t]
