"""Extended-precision reference for the device building blocks: irs_sincos and the Dual arithmetic (csrc/dual.hpp), the
four analytic model functors with the quadrotor's hand-derived Jacobian (csrc/models.hpp) and the Philox + Box-Muller
draw (csrc/philox.hpp).  Nothing here is taken from the code under test.

MODEL STEPS.  Restated from the equations oracle/irs_oracle.py restates, with the same citations into the reference
repository, over a generic number type: the same text runs on floats and on mpmath.mpf (DPS digits).  Sines and cosines
come from a `trig(k, angle)` callback, k numbering the model's angles, so that a reference evaluation can perturb one
sine or cosine VALUE and read off the step's sensitivity to it.  The three-cart branches are strict `<`.

DERIVATIVES.  Forward differences in mpmath with step FD = 1e-25 at DPS = 80 digits: J_fd(v) = J(v) + O(FD f''), and the
second derivatives, dJ/dv_l = (J_fd(v + FD e_l) - J_fd(v)) / FD, carry an O(FD) error too because the bias of J_fd is
smooth and cancels in the difference; round-off is 1e-80 / FD^2 = 1e-30.  The Jacobian used as the REFERENCE VALUE is the
central difference (error FD^2).  The three-cart step is differentiated on the branch the base point takes (the
derivative of the active branch, which is what the dual numbers give).

BOUNDS (bound()).  For a computed quantity g -- a component of the step or a Jacobian entry -- at v = (x, u):
    eps K (|g| + sum_l |dg/dv_l| |v_l|)  +  sum over the sines / cosines on the path: e_sincos |dg/d(that value)|
eps = 2^-24 (f32) or 2^-53 (f64); g and its derivatives from mpmath (for Jacobian entries: the second derivatives);
e_sincos = 1.5e-7 absolute in f32 (the number csrc/dual.hpp states for |x| < 1e3) and 2 ulp of the value in f64.  For the
Jacobian the perturbed pair is what a Dual carries: sin~ = sin + ds, cos~ = cos + dc, d sin~ = cos~ d(angle),
d cos~ = -sin~ d(angle) -- modelled as sin~(a) = sin a + ds + dc (a - a0), cos~(a) = cos a + dc - ds (a - a0).
K is the number of rounded operations on the longest path to an output, counted from csrc/models.hpp (one per +, -, *, /
and per parameter rounded to the scalar type; a sine or cosine is not counted: it has its own term):

    model       K step  K Jacobian   the longest path
    pendulum       6        6        xn[0]: T(h) | u - sin | h * | x1 + | h * | x0 +          (the partials ride the same
                                     chain: d sin = cos * 1, then one * or + per level)
    bicycle        6       13        xn[2]: T(h) | 1 / cs | ss * inv | x3 * | h * | x2 +      (Dual operator/: inv, r.v;
                                     Jacobian: + cs * 1, ss * 1 for d sin, d cos, r.v * b.d, a.d -, * inv (5), and the
                                     product rule of x3 * (.): a.d * b.v, a.v * b.d, + -- of which two on the path (2))
    three_cart    11       11        xn[0], all three stuck: T(h) | T(d) | h * u0 | x3 + | h * v1 | x0 + | + q2 | + q3 |
                                     T(1/3) | * | - d         (piecewise linear: the partials are constants on the chain)
    quadrotor     16       28        xn[9]: T(Ixx) | cr * cp | * rd2 | - sr * rd1 (rb) | Ixx * pb .. rb * (.) | - | M1 - |
                                     1 / Iyy | * iIyy (qd) | sr * tp .. * qd | four + of rr0 | h * | x9 +  = 16; the
                                     Jacobian adds two rounded operations (a product and a sum of the product rule) for
                                     each of the six multiplications on that path: 16 + 12 = 28, for the duals and for
                                     step_jac alike (it spells the same product rule out by hand)

RNG.  box_muller() is the specification of oracle.irs_oracle.device_gaussian_samples in mpmath.  The smoothing stream forms
u1 = (r + 0.5) / 2^32 in f32 (csrc/philox.hpp).  Next to 1 the f32 numbers are 2^-24 apart, so the rounded u1 is off by
at most half of that, |du1| <= 2^-25 (the conversion of r rounds to a multiple of 256 = 2^-24 2^32; the + 0.5 is absorbed),
and with d rad / d u1 = -1 / (u1 rad) for rad = sqrt(-2 ln u1):  |d rad| <= 2^-25 / (u1 rad) <= 2^-25 / rad (1 + 2^-20)
wherever the deviation matters (u1 > 1 - 2^-20; for smaller u1 the f32 spacing shrinks with u1 and the term is below the
tolerance it is added to).  When u1 rounds to exactly 1 the device radius is 0 and the deviation is rad itself:
    |d rad| <= min(rad, 2^-25 / rad (1 + 2^-20))                                    (rng_radius_deviation)
The angle is not affected: q / 4 and u2 - q / 4 are exact in f32.
"""
import json
import math
import os

import mpmath as mp
import numpy as np

from oracle import irs_oracle as orc

DPS = 80
FD = mp.mpf(10) ** -25
EPS = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
SINCOS_ABS_F32 = 1.5e-7        # csrc/dual.hpp, |x| < 1e3
SINCOS_ULP_F64 = 2.0           # csrc/dual.hpp, |x| < 1e6
# At the f64 neighbours of k pi/2 the result is as small as 4e-18 and the error of the reduction, absolute (the two-term
# split of pi/2 leaves ~1e-33 per quadrant; measured at most 3.9e-28 on results below 7e-13), is many ulp OF THAT
# RESULT: 450.94 ulp measured against mpmath over the points below (k = 29, x = 45.553093477052).  1.25 x that:
SINCOS_ULP_F64_NEIGHBOURS = 564.0
F32 = np.float32


# ---------------------------------------------------------------------------------------------------- the model steps
def pendulum_step(p, x, u, trig, branch=None):
    # examples/pendulum/pendulum_dynamics.py:46-60, semi-implicit Euler
    h = p[0]
    s, _ = trig(0, x[0])
    next_speed = x[1] + h * (-s + u[0])
    next_angle = x[0] + h * next_speed
    return [next_angle, next_speed]


def _matmul(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def _matvec(A, v):
    return [sum(A[i][k] * v[k] for k in range(3)) for i in range(3)]


def quadrotor_step(p, x, u, trig, branch=None):
    # examples/quadrotor/quadrotor_dynamics.py:40-77 (explicit Euler on an rpy rigid body); params :22-37
    h, mass, L, g, Ixx, Iyy, Izz, kF, kM = p[:9]
    uF = [kF * ui for ui in u]
    uM = [kM * ui for ui in u]
    Fz = uF[0] + uF[1] + uF[2] + uF[3]
    M = [L * (-uF[0] - uF[1] + uF[2] + uF[3]), L * (-uF[0] - uF[3] + uF[1] + uF[2]), -uM[0] + uM[1] - uM[2] + uM[3]]
    sr, cr = trig(0, x[3])
    sp, cp = trig(1, x[4])
    sy, cy = trig(2, x[5])
    rpy_d = [x[9], x[10], x[11]]
    # :150-186 R_WB = Rz Ry Rx
    Rx = [[1, 0, 0], [0, cr, -sr], [0, sr, cr]]
    Ry = [[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]]
    Rz = [[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]
    R = _matmul(Rz, _matmul(Ry, Rx))
    RF = _matvec(R, [0, 0, Fz])
    xyz_dd = [RF[0] / mass, RF[1] / mass, (RF[2] - mass * g) / mass]
    # :188-199 PhiInv, :59-61 Euler's equation
    PhiInv = [[1, 0, -sp], [0, cr, sr * cp], [0, -sr, cr * cp]]
    pqr = _matvec(PhiInv, rpy_d)
    inertia = [Ixx, Iyy, Izz]
    Iw = [inertia[i] * pqr[i] for i in range(3)]
    cross = [pqr[1] * Iw[2] - pqr[2] * Iw[1], pqr[2] * Iw[0] - pqr[0] * Iw[2], pqr[0] * Iw[1] - pqr[1] * Iw[0]]
    pqr_d = [(M[i] - cross[i]) / inertia[i] for i in range(3)]
    # :201-212 Phi, :215-231 Phi_d
    tp, cp2 = sp / cp, cp * cp
    Phi = [[1, sr * sp / cp, cr * sp / cp], [0, cr, -sr], [0, sr / cp, cr / cp]]
    D = [[[0, 0, 0] for _ in range(3)] for _ in range(3)]
    D[0][1] = [cr * tp, sr / cp2, 0]
    D[0][2] = [-sr * tp, cr / cp2, 0]
    D[1][1] = [-sr, 0, 0]
    D[1][2] = [-cr, 0, 0]
    D[2][1] = [cr / cp, sr * sp / cp2, 0]
    D[2][2] = [-sr / cp, cr * sp / cp2, 0]
    PD = [[sum(D[i][j][k] * rpy_d[k] for k in range(3)) for j in range(3)] for i in range(3)]
    a = _matvec(Phi, pqr_d)
    b = _matvec(PD, pqr)
    rpy_dd = [a[i] + b[i] for i in range(3)]
    xdot = [x[6], x[7], x[8], x[9], x[10], x[11]] + xyz_dd + rpy_dd
    return [x[i] + h * xdot[i] for i in range(12)]


def bicycle_step(p, x, u, trig, branch=None):
    # examples/bicycle/bicycle_dynamics.py:47-64
    h = p[0]
    sh, ch = trig(0, x[2])
    ss, cs = trig(1, x[4])
    dxdt = [x[3] * ch, x[3] * sh, x[3] * (ss / cs), u[0], u[1]]
    return [x[i] + h * dxdt[i] for i in range(5)]


def three_cart_branch(p, x, u):
    """(c12, c23) of examples/three_cart/three_cart_dynamics.py:44-46: strict `<` on the semi-implicit gaps."""
    h, d = p[0], p[1]
    v1s, v2s, v3s = x[3] + h * u[0], x[4], x[5] + h * u[1]
    q1s, q2s, q3s = x[0] + h * v1s, x[1] + h * v2s, x[2] + h * v3s
    return (q2s - q1s < d), (q3s - q2s < d)


def three_cart_step(p, x, u, trig, branch=None):
    # examples/three_cart/three_cart_dynamics.py:22-107 (the scalar `dynamics`); branch: the (c12, c23) to follow
    h, d = p[0], p[1]
    q1, q2, q3, v1, v2, v3 = x
    v1s, v2s, v3s = v1 + h * u[0], v2, v3 + h * u[1]
    q1s, q2s, q3s = q1 + h * v1s, q2 + h * v2s, q3 + h * v3s
    c12, c23 = three_cart_branch(p, x, u) if branch is None else branch
    third, half = x[0] * 0 + 1, x[0] * 0 + 1
    third, half = third / 3, half / 2
    if c12 and c23:
        q2n = third * (q1s + q2s + q3s)
        q1n, q3n = q2n - d, q2n + d
        v1n = v2n = v3n = third * (v1s + v2s + v3s)
    elif c12:
        pen = d - (q2s - q1s)
        q2n, q1n = q2s + half * pen, q1s - half * pen
        v1n = v2n = half * (v1s + v2s)
        q3n, v3n = q3s, v3s
    elif c23:
        pen = d - (q3s - q2s)
        q3n, q2n = q3s + half * pen, q2s - half * pen
        v2n = v3n = half * (v2s + v3s)
        q1n, v1n = q1s, v1s
    else:
        q1n, q2n, q3n, v1n, v2n, v3n = q1s, q2s, q3s, v1s, v2s, v3s
    return [q1n, q2n, q3n, v1n, v2n, v3n]


QUAD_PARAMS = [0.05, 0.775, 0.15, 9.81, 0.0015, 0.0025, 0.0035, 1.0, 0.0245]   # quadrotor_dynamics.py:22-37, h = 0.05
# name -> step, n, m, params (h first; the three-cart's h and d dyadic: its gap arithmetic is exact), the state indices
# of the angles in trig order, K of the table above, and the inputs the step is NOT affine in (only their second
# derivatives are formed; test_functors_cpu.py checks on one state per model that the others' vanish)
MODELS = {
    "pendulum": dict(step=pendulum_step, n=2, m=1, params=[0.05], angles=[0], K=(6, 6), curved=[0]),
    "quadrotor": dict(step=quadrotor_step, n=12, m=4, params=QUAD_PARAMS, angles=[3, 4, 5], K=(16, 28),
                      curved=[3, 4, 5, 9, 10, 11, 12, 13, 14, 15]),
    "bicycle": dict(step=bicycle_step, n=5, m=2, params=[0.1], angles=[2, 4], K=(6, 13), curved=[2, 3, 4]),
    "three_cart": dict(step=three_cart_step, n=6, m=2, params=[0.125, 0.25], angles=[], K=(11, 11), curved=[]),
}
SYSTEM_CLASSES = {"pendulum": ("PendulumDynamics", "PendulumOracle"), "quadrotor": ("QuadrotorDynamics", "QuadrotorOracle"),
                  "bicycle": ("BicycleDynamics", "BicycleOracle"), "three_cart": ("ThreeCartDynamics", "ThreeCartOracle")}


def float_trig(k, a):
    return math.sin(a), math.cos(a)


def step_float(name, x, u):
    """The restatement on plain floats (for the cross-check against the oracle classes)."""
    M = MODELS[name]
    return np.array(M["step"](M["params"], [float(v) for v in x], [float(v) for v in u], float_trig))


# ------------------------------------------------------------------------------------ reference values and sensitivities
def _split(vals):
    """mpf array -> (hi, lo) float64 arrays with hi + lo = the value to ~1e-32 relative."""
    hi = np.array([float(v) for v in vals])
    lo = np.array([float(v - mp.mpf(h)) for v, h in zip(vals, hi)])
    return hi, lo


_cache = {}


def reference(name, x, u, jac=True, all_inputs=False):
    """The mpmath reference at (x, u) (float arrays, taken exactly).  dict of float64 arrays:
    f_hi, f_lo (n)            the step, as a double-double
    cond_f (n)                |f_i| + sum_l |df_i/dv_l| |v_l|
    trig_val (na, 2)          sin, cos of the model's angles
    trig_f (n, na, 2)         |df_i / d(sin_k)|, |df_i / d(cos_k)|
    and with jac: J_hi, J_lo (n, d), cond_J (n, d) = |J_ij| + sum_l |dJ_ij/dv_l| |v_l|, trig_J (n, d, na, 2)."""
    key = (name, tuple(np.asarray(x, float)), tuple(np.asarray(u, float)), jac, all_inputs)
    if key in _cache:
        return _cache[key]
    M = MODELS[name]
    n, m, step = M["n"], M["m"], M["step"]
    d, na = n + m, len(M["angles"])
    with mp.workdps(DPS):
        p = [mp.mpf(v) for v in M["params"]]
        v0 = [mp.mpf(float(a)) for a in list(x) + list(u)]
        a0 = [v0[i] for i in M["angles"]]
        branch = three_cart_branch(p, v0[:n], v0[n:]) if name == "three_cart" else None

        def make_trig(pert=None):
            def trig(k, a):
                s, c = mp.sin(a), mp.cos(a)
                if pert is not None and pert[0] == k:
                    ds, dc = pert[1], pert[2]
                    s, c = s + ds + dc * (a - a0[k]), c + dc - ds * (a - a0[k])
                return s, c
            return trig

        def f_at(v, trig):
            return step(p, v[:n], v[n:], trig, branch)

        def J_fwd(v, trig, f0=None, only=None):
            """Forward-difference Jacobian; `only`: the columns to form (the others: 0)."""
            f0 = f_at(v, trig) if f0 is None else f0
            cols = []
            for j in range(d):
                if only is not None and j not in only:
                    cols.append([mp.mpf(0)] * n)
                    continue
                w = list(v)
                w[j] = w[j] + FD
                fj = f_at(w, trig)
                cols.append([(fj[i] - f0[i]) / FD for i in range(n)])
            return [[cols[j][i] for j in range(d)] for i in range(n)]

        # a column in which the step is affine with a constant coefficient does not move with v or with a sine: the
        # perturbed Jacobians are formed in the `curved` columns only (all_inputs: everywhere)
        curved = list(range(d)) if all_inputs else M["curved"]
        plain = make_trig()
        f0 = f_at(v0, plain)
        Jf = J_fwd(v0, plain, f0)
        absv = [abs(v) for v in v0]
        out = {}
        out["f_hi"], out["f_lo"] = _split(f0)
        out["cond_f"] = np.array([float(abs(f0[i]) + sum(abs(Jf[i][l]) * absv[l] for l in range(d))) for i in range(n)])
        out["trig_val"] = np.array([[float(mp.sin(a)), float(mp.cos(a))] for a in a0]).reshape(na, 2)
        trig_f = np.zeros((n, na, 2))
        trig_J = np.zeros((n, d, na, 2))
        for k in range(na):
            for sc in range(2):
                tr = make_trig((k, FD if sc == 0 else 0, FD if sc == 1 else 0))
                fk = f_at(v0, tr)
                trig_f[:, k, sc] = [float(abs((fk[i] - f0[i]) / FD)) for i in range(n)]
                if jac:
                    Jk = J_fwd(v0, tr, fk, curved)
                    trig_J[:, :, k, sc] = [[float(abs((Jk[i][j] - Jf[i][j]) / FD)) if j in curved else 0.0
                                            for j in range(d)] for i in range(n)]
        out["trig_f"] = trig_f
        if jac:
            Jc = []
            for i in range(n):
                Jc.append([None] * d)
            for j in range(d):
                wp, wm = list(v0), list(v0)
                wp[j], wm[j] = wp[j] + FD, wm[j] - FD
                fp, fm = f_at(wp, plain), f_at(wm, plain)
                for i in range(n):
                    Jc[i][j] = (fp[i] - fm[i]) / (2 * FD)
            hi, lo = _split([Jc[i][j] for i in range(n) for j in range(d)])
            out["J_hi"], out["J_lo"] = hi.reshape(n, d), lo.reshape(n, d)
            cond = [[abs(Jc[i][j]) for j in range(d)] for i in range(n)]
            for l in curved:
                if v0[l] == 0:
                    continue
                w = list(v0)
                w[l] = w[l] + FD
                Jl = J_fwd(w, plain, None, curved)
                for i in range(n):
                    for j in curved:
                        cond[i][j] += abs((Jl[i][j] - Jf[i][j]) / FD) * absv[l]
            out["cond_J"] = np.array([[float(c) for c in row] for row in cond])
            out["trig_J"] = trig_J
    _cache[key] = out
    return out


def _sincos_err(prec, trig_val):
    if prec == "f32":
        return np.full(trig_val.shape, SINCOS_ABS_F32)
    return SINCOS_ULP_F64 * np.array([[math.ulp(abs(v)) for v in row] for row in trig_val]).reshape(trig_val.shape)


def bound(name, ref, prec, what):
    """The allowed error of the step (`what` = "f", shape (n)) or of the Jacobian ("J", shape (n, d))."""
    K = MODELS[name]["K"][0 if what == "f" else 1]
    e = _sincos_err(prec, ref["trig_val"])
    return EPS[prec] * K * ref["cond_" + what] + (ref["trig_" + what] * e).sum(axis=(-2, -1))


def error(ref, got, what):
    """|got - reference| from the double-double reference (got - hi is exact where it matters)."""
    got = np.asarray(got, float)
    return np.abs((got - ref[what + "_hi"]) - ref[what + "_lo"])


def references(name, X, U, jac=True):
    return [reference(name, X[i], U[i], jac) for i in range(X.shape[0])]


def stack(refs, key):
    return np.stack([r[key] for r in refs])


# -------------------------------------------------------------------------------------------------------- state tables
Z_MAG = 2.0 ** -6       # the single sample of the device pass: z_c = sign(xs_c) 2^-6, so that xb = xs - z, xb + z = xs exactly


def sample_of(V):
    """z (same shape, f32) for table rows V = [xs | us]: sign(v) 2^-6 (+ for 0)."""
    return np.where(np.signbit(V), -Z_MAG, Z_MAG).astype(F32)


def _snap(V):
    """Rows moved (by at most an ulp of 2^-6) so that both v - z and (v - z) + z are exact in f32."""
    V = np.asarray(V, F32) + F32(0.0)       # (-0 -> +0)
    z = sample_of(V)
    vb = (V - z).astype(F32)
    vs = (vb + z).astype(F32)
    assert np.array_equal(vb.astype(np.float64) + z.astype(np.float64), vs.astype(np.float64))
    assert np.array_equal(sample_of(vs), z)
    return vs


def _near(rs, k, center_sign, lo, hi):
    """k angles +-(pi/2 - delta), delta uniform in [lo, hi)."""
    delta = lo + (hi - lo) * rs.rand(k)
    return center_sign * (math.pi / 2 - delta)


def _signs(rs, k):
    return np.where(rs.rand(k) < 0.5, -1.0, 1.0)


def _logmag(rs, k, lo, hi):
    return _signs(rs, k) * np.exp(rs.uniform(math.log(lo), math.log(hi), k))


def _f32_neighbours(vals):
    c = np.asarray(vals, np.float64).astype(F32)
    return np.concatenate([np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))])


def tables(name):
    """{regime: V (k, n + m) f32 rows [x | u]}, deterministic (numpy's frozen RandomState), every entry exact in f32 and
    placed so that the nominal point xb = xs - sample_of(xs) of the device pass is exact too."""
    rs = np.random.RandomState({"pendulum": 11, "quadrotor": 12, "bicycle": 13, "three_cart": 14}[name])
    T = {}
    if name == "pendulum":
        for lo, tag in ((1e-2, "theta_1e-2"), (1e-1, "theta_1e-1"), (1.0, "theta_1e0"), (10.0, "theta_1e1"), (100.0, "theta_1e2")):
            k = 24
            T[tag] = np.column_stack([_logmag(rs, k, lo, 10 * lo * 0.999), 2 * rs.randn(k), rs.randn(k)])
        ks = np.array([1, 2, 3, 4, 5, 7, 100, 201, 402, 636])
        th = _f32_neighbours(np.concatenate([ks, -ks]) * (math.pi / 2))
        T["k_pi_2"] = np.column_stack([th, 2 * rs.randn(th.size), rs.randn(th.size)])
        return {k: _snap(v) for k, v in T.items()}
    if name == "quadrotor":
        def base(k):
            x = 0.5 * rs.randn(k, 12)
            u = 2.0 + 0.5 * rs.randn(k, 4)
            return x, u
        x, u = base(16)
        T["moderate"] = np.hstack([x, u])
        for tag, lo, hi in (("pitch_0.3", 0.1, 0.3), ("pitch_0.1", 0.01, 0.1), ("pitch_1e-2", 0.001, 0.01)):
            x, u = base(16)
            x[:, 4] = _near(rs, 16, _signs(rs, 16), lo, hi)
            T[tag] = np.hstack([x, u])
        x, u = base(16)
        x[:, 3], x[:, 5] = _logmag(rs, 16, 1.0, 999.0), _logmag(rs, 16, 1.0, 999.0)
        T["roll_yaw_1e3"] = np.hstack([x, u])
        x, u = base(16)
        x[:8, 9:12] = 0.0
        x[8:, 9:12] = 20.0 * rs.randn(8, 3)
        T["rates_0_large"] = np.hstack([x, u])
        x, u = base(8)
        u[:] = 0.0
        T["zero_thrust"] = np.hstack([x, u])
        return {k: _snap(v) for k, v in T.items()}
    if name == "bicycle":
        def base(k):
            x = rs.randn(k, 5) * np.array([2.0, 2.0, 1.0, 2.0, 0.4])
            return x, rs.randn(k, 2)
        x, u = base(32)
        T["moderate"] = np.hstack([x, u])
        for tag, lo, hi in (("steer_0.1", 0.01, 0.1), ("steer_1e-2", 0.001, 0.01)):
            x, u = base(32)
            x[:, 4] = _near(rs, 32, _signs(rs, 32), lo, hi)
            T[tag] = np.hstack([x, u])
        x, u = base(32)
        x[:16, 3] = 0.0
        x[16:, 3] = -np.abs(x[16:, 3]) - 0.5
        T["speed_0_neg"] = np.hstack([x, u])
        x, u = base(32)
        x[:, 2] = _logmag(rs, 32, 1.0, 999.0)
        T["heading_1e3"] = np.hstack([x, u])
        return {k: _snap(v) for k, v in T.items()}
    # three-cart: h = 2^-3, d = 2^-2.  Interior rows: multiples of 2^-6 below 8, so every sum of the step is exact; gaps at
    # least 2^-4 from d.
    h, d = MODELS[name]["params"]

    def interior(k, want):
        rows = []
        while len(rows) < k:
            x = np.round(rs.uniform(-2, 2, 6) * 64) / 64
            u = np.round(rs.uniform(-2, 2, 2) * 64) / 64
            g12 = 0.5 * rs.rand() if want[0] else 0.5 + 0.5 * rs.rand()
            g23 = 0.5 * rs.rand() if want[1] else 0.5 + 0.5 * rs.rand()
            # place q2, q3 from the semi-implicit positions so that the gaps are g d (rounded to 2^-10)
            v1s, v3s = x[3] + h * u[0], x[5] + h * u[1]
            q1s = x[0] + h * v1s
            g12, g23 = np.round(g12 * 2 * d * 1024) / 1024, np.round(g23 * 2 * d * 1024) / 1024
            if abs(g12 - d) < 1 / 16 or abs(g23 - d) < 1 / 16:
                continue
            x[1] = q1s + g12 - h * x[4]
            x[2] = x[1] + h * x[4] + g23 - h * v3s
            rows.append(np.concatenate([x, u]))
        return np.array(rows)
    for tag, want in (("stuck_123", (True, True)), ("contact_12", (True, False)), ("contact_23", (False, True)),
                      ("free", (False, False))):
        T[tag] = interior(16, want)
    # switching surfaces: cart 2 arrives at q2* = 0 (q2 = -h v2), carts 1 and 3 rest at -g12 and +g23 with u = 0, so the
    # gaps are g12 and g23 exactly, in f32 and in f64.  Each gap takes d itself, its f32 neighbours d (1 -+ 2^-24 | 2^-23)
    # and d -+ 1/8.
    dd = F32(d)
    gaps = [np.nextafter(dd, F32(0)), dd, np.nextafter(dd, F32(1)), F32(d - 0.125), F32(d + 0.125)]
    rows = [[-g12, -h * v2, g23, 0.0, v2, 0.0, 0.0, 0.0] for v2 in (0.0, 0.5, -0.25) for g12 in gaps for g23 in gaps]
    T["surface"] = np.array(rows, np.float64)
    out = {k: _snap(v) for k, v in T.items()}
    for k, v in T.items():      # nothing moved: the interior rows and the surfaces are where they were put
        assert np.array_equal(out[k].astype(np.float64), v), k
    return out


def three_cart_gaps(V):
    """The semi-implicit gaps (g12, g23) of three-cart rows in exact rational arithmetic (as mpf)."""
    h, d = MODELS["three_cart"]["params"]
    out = []
    with mp.workdps(DPS):
        for r in V:
            x, u = [mp.mpf(float(a)) for a in r[:6]], [mp.mpf(float(a)) for a in r[6:]]
            v1s, v3s = x[3] + h * u[0], x[5] + h * u[1]
            q1s, q2s, q3s = x[0] + h * v1s, x[1] + h * x[4], x[2] + h * v3s
            out.append((q2s - q1s, q3s - q2s))
    return out


# ------------------------------------------------------------------------------------------------------ sincos points
def sincos_points():
    """(x32 f32 array with |x| < 1e3, x64 f64 array with |x| < 1e6, mask of the x64 that are neighbours of a multiple of
    pi/4): per decade a deterministic sweep, the neighbours of
    k pi/2 and of (k + 1/2) pi/2 (every k to 64, then a spread of k up to the domain limit), +-0, denormals and the
    smallest normals."""
    rs = np.random.RandomState(5)

    def family(kmax, dtype, extra):
        ks = np.unique(np.concatenate([np.arange(1, 65), np.round(np.exp(rs.uniform(math.log(64), math.log(kmax), extra))),
                                       [kmax]])).astype(np.float64)
        pts = []
        with mp.workdps(40):
            for k in ks:
                for half in (0, 1):
                    c = dtype(float((mp.mpf(k) + mp.mpf(half) / 2) * mp.pi / 2))
                    pts += [np.nextafter(c, dtype(-np.inf)), c, np.nextafter(c, dtype(np.inf))]
        pts = np.array(pts, dtype)
        return np.concatenate([pts, -pts])
    sweep32 = np.concatenate([_logmag(rs, 400, 10.0 ** e, 10.0 ** (e + 1)) for e in range(-6, 3)]).astype(F32)
    edge32 = np.array([0.0, -0.0, 1e-45, -1e-45, 5.9e-39, 1.17549435e-38, -1.17549435e-38, 1e-30], F32)
    x32 = np.concatenate([sweep32, family(636, F32, 400), edge32])
    x32 = x32[np.abs(x32) < 1e3]
    sweep64 = np.concatenate([_logmag(rs, 300, 10.0 ** e, 10.0 ** (e + 1)) for e in range(-6, 6)])
    edge64 = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e-300])
    fam64 = family(636619, np.float64, 600)
    x64 = np.concatenate([sweep64, fam64, edge64])
    near = np.concatenate([np.zeros(sweep64.size, bool), np.ones(fam64.size, bool), np.zeros(edge64.size, bool)])
    keep = np.abs(x64) < 1e6
    return x32, x64[keep], near[keep]


def sincos_reference(x):
    """(sin, cos) of float points as double-doubles: arrays (k, 2) hi and lo."""
    with mp.workdps(60):
        vals = []
        for v in np.asarray(x, np.float64):
            a = mp.mpf(float(v))
            vals += [mp.sin(a), mp.cos(a)]
        hi, lo = _split(vals)
    return hi.reshape(-1, 2), lo.reshape(-1, 2)


# -------------------------------------------------------------------------------------------------------------- RNG
RNG_SEED, RNG_IT = 0x5EED0F1CE, 3          # the (seed, iteration) whose t = 0, j = 0 stream is scanned
RNG_SCAN = 1 << 24
RNG_GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "rng_extremes.json")
RNG_U2_TARGETS = [(k, 8) for k in range(9)]       # k/8: the quadrant boundaries k/4 and the rintf ties (2k+1)/8


def philox_words(indices, seed=RNG_SEED, it=RNG_IT, t=0, j=0):
    """The four Philox words of sample indices (csrc/philox.hpp: counter (index lo, t, j | index hi << 8, it))."""
    idx = np.asarray(indices, np.uint64)
    ctr = np.zeros((idx.size, 4), np.uint32)
    ctr[:, 0] = (idx & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[:, 1] = t
    ctr[:, 2] = np.uint32(j) | ((idx >> np.uint64(32)).astype(np.uint32) << np.uint32(8))
    ctr[:, 3] = it
    return orc.philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def scan_rng_extremes(count=RNG_SCAN, keep=16, chunk=1 << 20):
    """The sample indices below `count` with the `keep` smallest and largest u1 words (word 0) and, per target k/8, the
    `keep` u2 words (word 1) nearest k/8 2^32."""
    w0, w1 = np.empty(count, np.uint32), np.empty(count, np.uint32)
    for a in range(0, count, chunk):
        w = philox_words(np.arange(a, min(count, a + chunk), dtype=np.uint64))
        w0[a:a + w.shape[0]], w1[a:a + w.shape[0]] = w[:, 0], w[:, 1]
    order = np.argsort(w0, kind="stable")
    out = {"seed": RNG_SEED, "it": RNG_IT, "scanned": count,
           "u1_smallest": [int(i) for i in order[:keep]], "u1_largest": [int(i) for i in order[::-1][:keep]]}
    u2 = (w1.astype(np.float64) + 0.5) / 4294967296.0
    for k, den in RNG_U2_TARGETS:
        near = np.argsort(np.abs(u2 - k / den), kind="stable")[:keep]
        out["u2_near_%d_%d" % (k, den)] = [int(i) for i in near]
    return out


def rng_extremes():
    with open(RNG_GOLDEN) as f:
        return json.load(f)


def rng_extreme_indices(g):
    return sorted({i for k, v in g.items() if isinstance(v, list) for i in v})


def box_muller(words):
    """The specification (oracle.irs_oracle.device_gaussian_samples) in mpmath: words (k, 4) uint32 -> z (k, 4) float64,
    rad (k, 2) float64."""
    z, rad = np.zeros((len(words), 4)), np.zeros((len(words), 2))
    with mp.workdps(50):
        for i, w in enumerate(words):
            for pr in range(2):
                u1 = (mp.mpf(int(w[2 * pr])) + mp.mpf(1) / 2) / 4294967296
                u2 = (mp.mpf(int(w[2 * pr + 1])) + mp.mpf(1) / 2) / 4294967296
                r = mp.sqrt(-2 * mp.log(u1))
                rad[i, pr] = float(r)
                z[i, 2 * pr], z[i, 2 * pr + 1] = float(r * mp.cos(2 * mp.pi * u2)), float(r * mp.sin(2 * mp.pi * u2))
    return z, rad


def rng_radius_deviation(rad):
    """|d rad| the smoothing stream is allowed from forming u1 in f32 (derivation in the module docstring)."""
    rad = np.asarray(rad, float)
    return np.minimum(rad, 2.0 ** -25 / np.maximum(rad, 1e-300) * (1 + 2.0 ** -20))


def rng_tolerance(z, rad, exact_tail):
    """Element-wise tolerance on z (k, 4): rtol 2e-5 / atol 2e-6 (tests/test_gpu_parity.py), plus, for the smoothing
    stream, the radius deviation (|cos|, |sin| <= 1)."""
    tol = 2e-5 * np.abs(z) + 2e-6
    return tol if exact_tail else tol + np.repeat(rng_radius_deviation(rad), 2, axis=1)


def box_muller_f32(words):
    """The smoothing stream's draw emulated in numpy f32: u1, u2 formed in f32, log / sqrt / sin / cos correctly rounded
    from f64 (the device's are within a few f32 ulp of these)."""
    w = np.asarray(words, np.uint32)
    z = np.zeros((w.shape[0], 4), F32)
    for pr in range(2):
        u1 = ((w[:, 2 * pr].astype(F32) + F32(0.5)) * F32(2.3283064365386963e-10)).astype(F32)
        u2 = ((w[:, 2 * pr + 1].astype(F32) + F32(0.5)) * F32(2.3283064365386963e-10)).astype(F32)
        rad = np.sqrt((F32(-2.0) * np.log(u1.astype(np.float64)).astype(F32)).astype(np.float64)).astype(F32)
        q = np.rint(F32(4.0) * u2).astype(F32)
        r = ((u2 - F32(0.25) * q).astype(F32) * F32(6.283185307179586)).astype(F32)
        ang = r.astype(np.float64) + q.astype(np.float64) * (math.pi / 2)
        z[:, 2 * pr] = (rad * np.cos(ang).astype(F32)).astype(F32)
        z[:, 2 * pr + 1] = (rad * np.sin(ang).astype(F32)).astype(F32)
    return z
