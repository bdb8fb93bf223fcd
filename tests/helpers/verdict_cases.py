"""The problems on which the descents' verdicts are pinned (include/irs_hip.h, rules V1 and V2): for V1, TV-LQR problems
with exactly one step t* whose control Hessian is not positive definite in the backward sweep; for V2, healthy problems
with one NaN or +Inf planted in the data.  tests/test_descent_verdicts_cpu.py admits every V1 case by the
extended-precision pivot trace of oracle/tvlqr_highprec.py; tests/test_descent_verdicts_gpu.py runs them.

V1, plain form (irs_tvlqr_riccati, irs_tvlqr_descent[_batch]; H_t = alpha R + B_t'P B_t).  R has ONE negative direction v,
alpha R = V diag(-NEG/2, 1/2, ..) V', and B_{t*} = 0: at t* the Hessian is alpha R itself, indefinite; at every other
step B_t'P B_t covers the small negative direction.  v runs over every e_j (the failing pivot of the LDL' moves with it: a
kernel that inspects one pivot cannot pass) and one rotated direction; t* over the first step of the sweep (T - 1), a
middle one and the last (0).

V1, ADMM form (H_t = alpha R + rho/2 Mu + B_t'P B_t, P carrying rho/2 Mx).  The same construction with the negative
direction sized against rho/2 on a bounded control: R_jj = -(rho + NEG) there, so that alpha R_jj + rho/2 = -NEG/2 again;
and along an unbounded control, where no penalty is added.

V1, position-controlled form (irs_quasistatic_box_descent, solvers 1, 2, 3 and the batch; augmented state [x; u_prev],
B~ = [B; I], cost du'R du).  A concave state cost (-CONC Q, -CONC Qd), B_t = 0 for t > t* -- the state is out of the
controls' reach there, du = 0 is optimal, P_uu stays (the penalty's) and H_t = R (+ rho/2) is positive definite --
and a B_{t*} of full rank whose column j is of order one and whose other columns are scaled by 1e-3: B~'P B~ then has one
large negative direction near e_j, so the failing pivot of the closed-form inverse (p, det, the Schur block's p and det)
moves with j.  Bounds: a box of +-0.05 around the start position (or on du).  The first backward sweep of every solver
starts from the empty active set and factors the full Hessian at every step, whatever the box; on the steps t > t* no
bound can bind in any later sweep either (du = 0 there); and the verdict latches at the first failure.  Below t* the
"plan" of an indefinite QP is garbage, and the box is what keeps the controls that reach the contact plant sane.

V2.  A healthy problem of each form -- one on which the entry reports the all-clear, which the GPU test asserts on the
clean twin first, so that the poisoned verdict is not vacuous -- and one poison in {NaN, +Inf} at a mid-horizon step of
At, Bt, ct, xd_trj, or in x0.
"""
import functools

import numpy as np

from oracle import irs_oracle as orc
from oracle import tvlqr_highprec as hp

NEG = 1e-3            # alpha R's eigenvalue along the planted direction is -NEG / 2 (its others: 1 / 2)
CONC = 100.0          # the concave state cost of the position-controlled cases: -CONC Q, -CONC Qd
RHO = 0.1             # the ADMM penalty of these cases: small against H, so that a healthy tail settles in a few iterations
MARGIN = 1e-6         # admission: |lambda_min(H_t)| > MARGIN max|H_t|, on the right side of zero (ten decades above f64 rounding)
MAX_ITER = 50         # a tail that cannot converge ends quickly
EPS = 1e-8

# (n, m, T, implementation): every path of irs_tvlqr_riccati at the smallest horizon that selects it (csrc/tvlqr.hip,
# riccati_backward_any: the matrix-core sizes fall back to the LDS recursion beyond (T + 1) n = 4096)
RICCATI_PATHS = ((2, 1, 6, "registers"), (5, 2, 8, "mfma"), (7, 4, 8, "mfma"), (12, 4, 8, "mfma"), (12, 4, 341, "lds"),
                 (3, 2, 9, "generic"), (16, 4, 6, "generic"))
# (model, h, T, implementation of its Riccati pass): irs_tvlqr_descent and its batch
DESCENT_PATHS = (("pendulum", 0.05, 6, "registers"), ("bicycle", 0.1, 8, "mfma"), ("quadrotor", 0.05, 8, "mfma"),
                 ("quadrotor", 0.05, 341, "lds"))
ADMM_MODEL = ("bicycle", 0.1, 8)          # irs_tvlqr_box_descent: control 0 bounded, control 1 unbounded
VALUES_SIZE = (3, 2, 9)                   # irs_box_values_begin: a size with no compiled kernel
DU_MODELS = ("box_pivoting", "planar_hand")       # M = 2 and M = 4: the closed-form branches of csrc/ctrlbox_mfma.hip
DU_T = 8
POISONS = {"nan": np.nan, "inf": np.inf}
FIELDS = ("At", "Bt", "ct", "xd", "x0")


def t_stars(T):
    """The first step of the backward sweep, a middle one, the last."""
    return (T - 1, T // 2, 0)


def directions(m):
    """e_0 .. e_{m-1} and, where there is room to rotate, one rotated direction."""
    return ["e%d" % j for j in range(m)] + (["rot"] if m > 1 else [])


def bad_R(m, direction, bounded=(), rho=0.0):
    """R with alpha_R R = V diag(-NEG/2, 1/2, ..) V' at alpha_R = 1/2: eigenvalue -NEG along `direction`, 1 along the
    others.  e_j on a control in `bounded`: R_jj = -(rho + NEG), which the ADMM's rho/2 brings back to -NEG/2."""
    d = np.ones(m)
    if direction == "rot":
        d[0] = -NEG
        V = hp._rotation(np.random.default_rng([m, 77]), m)
        R = (V * d).dot(V.T)
        return 0.5 * (R + R.T)
    j = int(direction[1:])
    d[j] = -(NEG + (rho if j in bounded else 0.0))
    return np.diag(d)


def _copy(p, keys=("At", "Bt", "ct", "xd", "x0", "Q", "Qd")):
    return {k: np.array(p[k], float, copy=True) for k in keys}


# ------------------------------------------------------------------------------------------------ V1, plain form
def plain_case(n, m, T, t_star, direction):
    """irs_tvlqr_riccati's case: oracle/tvlqr_highprec.py's dense conformance problem of the size, R replaced, B_{t*} = 0."""
    c = _copy(hp.riccati_problem(n, m, T, "spd"))
    c["Bt"][t_star] = 0.0
    c.update(R=bad_R(m, direction), alpha_R=0.5, T=T, t_star=t_star)
    return c


def descent_case(name, h, T, t_star, direction, B=3):
    """irs_tvlqr_descent's case and its batch: the model's own linearisation (hp.model_problem), B copies with the start
    and the goal shifted per problem; `single` is the failing problem (the middle one of the batch), whose B_{t*} = 0."""
    p = hp.model_problem(name, h, T)
    m = p["Bt"].shape[2]
    rng = np.random.default_rng([T, B, 5])
    n = p["x0"].shape[0]
    batch = dict(At=np.stack([p["At"]] * B), Bt=np.stack([p["Bt"]] * B), ct=np.stack([p["ct"]] * B),
                 xd=np.stack([p["xd"] + 0.01 * rng.normal(size=n) for _ in range(B)]),
                 x0=np.stack([p["x0"] + 0.01 * rng.normal(size=n) for _ in range(B)]))
    bad = B // 2
    batch["Bt"][bad, t_star] = 0.0
    shared = dict(Q=np.array(p["Q"]), Qd=np.array(p["Qd"]), R=bad_R(m, direction), alpha_R=0.5, T=T, t_star=t_star)
    return dict(batch=batch, bad=bad, name=name, h=h, **shared)


def problem_of(case, b):
    """Problem b of a batched case as a single problem."""
    out = {k: case["batch"][k][b] for k in ("At", "Bt", "ct", "xd", "x0")}
    out.update({k: case[k] for k in ("Q", "Qd", "R", "alpha_R", "T", "t_star")})
    return out


# ------------------------------------------------------------------------------------------------ V1, ADMM form
def admm_box(m, B=None):
    """Control 0 bounded (finite, never reached by a healthy plan), the others unbounded; no state bound.
    With the negative direction ON the bounded control (e0) the QP of every problem of the launch is concave along it
    inside the box -- only the penalised Hessian is positive definite, by about B'PB ~ 1e-2 -- and the ADMM iteration
    of the neighbours amplifies instead of settling: their verdict is then "not converged", and after 50 amplifying
    iterations per tail their realised cost overflows (info[0] = T + 1).  That is the right verdict on such a
    problem; what V1 asks of the neighbours there is their bits.  Along e1, the unbounded control, they are healthy."""
    ulo, uhi = np.full(m, -np.inf), np.full(m, np.inf)
    ulo[0], uhi[0] = -1e3, 1e3
    return (ulo, uhi) if B is None else (np.tile(ulo, (B, 1)), np.tile(uhi, (B, 1)))


def admm_case(t_star, direction, B=3):
    """irs_tvlqr_box_descent and its wsx / adaptive / lazy / batch entries: descent_case of the bicycle, the negative
    direction sized against rho/2 where it lies on the bounded control."""
    name, h, T = ADMM_MODEL
    c = descent_case(name, h, T, t_star, direction, B)
    m = c["R"].shape[0]
    c["R"] = bad_R(m, direction, bounded=(0,), rho=RHO)
    c.update(rho=RHO, pen_u=np.array([1.0] + [0.0] * (m - 1)), pen_x=np.zeros(c["Q"].shape[0]))
    return c


def values_case(t_star, direction):
    """irs_box_values_begin: plain_case of a size without a compiled kernel under admm_case's box."""
    n, m, T = VALUES_SIZE
    c = plain_case(n, m, T, t_star, direction)
    c["R"] = bad_R(m, direction, bounded=(0,), rho=RHO)
    c.update(rho=RHO, pen_u=np.array([1.0] + [0.0] * (m - 1)), pen_x=np.zeros(n))
    return c


# ------------------------------------------------------------------------------------------------ position-controlled form
def du_start(model):
    """(oracle system, a start state in contact, indices_u_into_x)."""
    if model == "planar_hand":
        sys_o = orc.PlanarHandOracle(0.1)
        x0 = orc.PlanarHandOracle.pack([0.0, 0.35, 0.0], [-np.pi / 4, -np.pi / 4], [np.pi / 4, np.pi / 4])
        for _ in range(4):
            x0 = sys_o.dynamics(x0, np.array([-np.pi / 4, -np.pi / 4, np.pi / 4, np.pi / 4]))
    elif model == "box_pivoting":
        sys_o = orc.BoxPivotOracle(0.1)
        x0 = orc.BoxPivotOracle.pack([0.0, 0.5, 0.0], [-0.5, 0.5])
        x0 = sys_o.dynamics(x0, np.array([-0.5, 0.5]))
    else:
        raise ValueError(model)
    return sys_o, x0, np.asarray(sys_o.indices_u_into_x)


def _du_rows(x0, idx, T, B, kind, width=0.05):
    """(lo, hi) rows (B,T,m): a box of +-width around the start position (kind "abs") or on du (kind "rel")."""
    m = len(idx)
    mid = np.tile(x0[..., idx][:, None, :], (1, T, 1)) if kind == "abs" else np.zeros((B, T, m))
    return mid - width, mid + width


@functools.lru_cache(maxsize=None)
def _du_start_cached(model):
    return du_start(model)


def du_case(model, t_star, j, B=3):
    """V1: B problems sharing the concave weights (Q, Qd, R are shared by a launch); the neighbours' B_t vanish at
    EVERY step, so all their Hessians are R: positive definite, their plan du = 0.  Problem B // 2 has the full-rank
    B_{t*} with column j of order one, and B_t of order 0.1 below t*."""
    sys_o, x0, idx = _du_start_cached(model)
    n, m, T = len(x0), len(idx), DU_T
    rng = np.random.default_rng([DU_MODELS.index(model), t_star, j])
    At = np.tile(np.eye(n), (B, T, 1, 1)) + 0.05 * rng.normal(size=(B, T, n, n))
    Bt = np.zeros((B, T, n, m))
    bad = B // 2
    scale = np.full(m, 1e-3)
    scale[j] = 1.0
    Bt[bad, t_star] = rng.normal(size=(n, m)) * scale
    Bt[bad, :t_star] = 0.1 * rng.normal(size=(t_star, n, m))
    ct = 0.01 * rng.normal(size=(B, T, n))
    x0s = np.tile(x0, (B, 1))
    xd = np.tile(x0, (B, T + 1, 1)) + 0.01 * rng.normal(size=(B, 1, n))
    batch = dict(At=At, Bt=Bt, ct=ct, xd=xd, x0=x0s)
    return dict(batch=batch, bad=bad, model=model, idx=idx, Q=-CONC * np.eye(n), Qd=-CONC * np.eye(n), R=np.eye(m),
                alpha_R=1.0, T=T, t_star=t_star, rho=RHO,
                rows={k: _du_rows(x0s, idx, T, B, k) for k in ("abs", "rel")})


def du_healthy(model, B=3):
    """V2's healthy problems: convex weights and the model's OWN linearisation (the exact one of the contact step,
    along the rollout that holds the start position), the goals 1e-3 off the start state.  A linearisation the plant
    does not follow would have every tail push against its box -- the realised state never goes where the plan says --
    and the ADMM run past its 50 iterations; on these the oracle's ADMM (orc.local_descent_quasistatic, rho = RHO, eps =
    EPS) needs at most 37 per tail under either box, and the active-set solvers a handful."""
    sys_o, x0, idx = _du_start_cached(model)
    n, m, T = len(x0), len(idx), DU_T
    rng = np.random.default_rng([DU_MODELS.index(model), 99])
    u_trj = np.tile(x0[idx], (T, 1))
    A, Bm, c = orc.exact_contact_TV(sys_o, orc.rollout(sys_o, x0, u_trj), u_trj)
    batch = dict(At=np.stack([A] * B), Bt=np.stack([Bm] * B), ct=np.stack([c] * B),
                 xd=np.tile(x0, (B, T + 1, 1)) + 1e-3 * rng.normal(size=(B, 1, n)), x0=np.tile(x0, (B, 1)))
    return dict(batch=batch, bad=B // 2, model=model, idx=idx, Q=np.eye(n), Qd=10.0 * np.eye(n), R=np.eye(m), alpha_R=1.0,
                T=T, t_star=None, rho=RHO, rows={k: _du_rows(batch["x0"], idx, T, B, k) for k in ("abs", "rel")})


def du_penalties(case, kind, solver):
    """(pen_x, pen_u) of the augmented problem: the ADMM (solver 1) penalises the bounded components -- the u_prev block
    of the state under an absolute box, the control du under a rate box; the active-set solvers penalise nothing."""
    n, m = case["Q"].shape[0], case["R"].shape[0]
    pen_x, pen_u = np.zeros(n + m), np.zeros(m)
    if solver == 1:
        if kind == "abs":
            pen_x[n:] = 1.0
        else:
            pen_u[:] = 1.0
    return pen_x, pen_u


# ------------------------------------------------------------------------------------------------ the traces
def trace(p, half_rho=0.0, pen_x=None, pen_u=None):
    """(t_bad, margins {t: lambda_min / max|H|}) of a single plain-form problem."""
    t_bad, H = hp.pivot_trace(p["At"], p["Bt"], p["Q"], p["Qd"], p["R"], p["alpha_R"], half_rho=half_rho, pen_x=pen_x,
                              pen_u=pen_u)
    return t_bad, {t: hp.definiteness_margin(h) for t, h in H.items()}


def trace_du(p, control, half_rho=0.0, pen_x=None, pen_u=None):
    """The same for a position-controlled problem in one of its two spellings (hp.position_controlled_form)."""
    f = hp.position_controlled_form(p["At"], p["Bt"], p["Q"], p["Qd"], p["R"], control)
    t_bad, H = hp.pivot_trace(f["At"], f["Bt"], f["Q"], f["Qd"], f["R"], 1.0, cross=f["cross"], half_rho=half_rho,
                              pen_x=pen_x, pen_u=pen_u)
    return t_bad, {t: hp.definiteness_margin(h) for t, h in H.items()}


def admitted(t_bad, margins, t_star, T):
    """The admission condition: the sweep stops at t*, every Hessian before it (t > t*) is positive definite by MARGIN,
    the one at t* indefinite by MARGIN.  t_star = None: a healthy problem, every step positive definite by MARGIN."""
    if t_star is None:
        return t_bad is None and len(margins) == T and min(margins.values()) > MARGIN
    return (t_bad == t_star and sorted(margins) == list(range(t_star, T)) and margins[t_star] < -MARGIN
            and all(margins[t] > MARGIN for t in range(t_star + 1, T)))


# ------------------------------------------------------------------------------------------------ V2
def healthy_plain(n, m, T):
    c = _copy(hp.riccati_problem(n, m, T, "spd"))
    c.update(R=np.array(hp.riccati_problem(n, m, T, "spd")["R"]), alpha_R=0.5, T=T, t_star=None)
    return c


def healthy_descent(name, h, T, B=3):
    c = descent_case(name, h, T, 0, "e0", B)
    p = hp.model_problem(name, h, T)
    c["batch"]["Bt"] = np.stack([p["Bt"]] * B)
    c.update(R=np.array(p["R"]), t_star=None)
    return c


def healthy_admm(B=3):
    name, h, T = ADMM_MODEL
    c = healthy_descent(name, h, T, B)
    m = c["R"].shape[0]
    c.update(rho=RHO, pen_u=np.array([1.0] + [0.0] * (m - 1)), pen_x=np.zeros(c["Q"].shape[0]))
    return c


def healthy_values():
    n, m, T = VALUES_SIZE
    c = healthy_plain(n, m, T)
    c.update(rho=RHO, pen_u=np.array([1.0] + [0.0] * (m - 1)), pen_x=np.zeros(n))
    return c


def poisoned(p, field, poison):
    """A copy of the single problem p with one element of `field` replaced: a mid-horizon step of the time-varying
    data (an off-diagonal element of A_t), the first component of x0."""
    q = dict(p)
    a = np.array(p[field], float, copy=True)
    tm = p["T"] // 2
    if field == "x0":
        a[0] = POISONS[poison]
    elif field == "At":
        a[tm, 0, 1 % a.shape[2]] = POISONS[poison]
    elif field == "Bt":
        a[tm, 0, 0] = POISONS[poison]
    else:
        a[tm, 0] = POISONS[poison]
    q[field] = a
    return q


def poisoned_batch(case, field, poison):
    """A copy of a batched case whose middle problem is poisoned."""
    out = dict(case)
    out["batch"] = {k: np.array(v, float, copy=True) for k, v in case["batch"].items()}
    b = case["bad"]
    out["batch"][field][b] = poisoned(problem_of(case, b), field, poison)[field]
    return out
