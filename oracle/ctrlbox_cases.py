"""The quasistatic descents on which the active-set kernels (csrc/ctrlbox.hip, lanes; csrc/ctrlbox_mfma.hip, tiles and
the batched entry) are certified: every position-controlled model, both kinds of control box, under bound rows that
differ per step, per component and per side, hold infinities, pin entries (lo == hi) or exclude the nominal.

A case is a deterministic function of its id "<model>-<kind>-<shape>-T<T>":

  model  hand (7, 4), pivot (5, 2), push (5, 2), bob = box-on-box (2, 1): the start states, goals and weights of
         test_quasistatic_descent_outputs_are_self_consistent (box-on-box: h = 0.1, m = 1, k = 100, start [0.9, 1.0],
         Q on the box only).  The nominal is x0[idx] plus a seeded random walk, (A, B, c) come from
         zero_order_B_decoupled of the oracle's contact step on 300 seeded samples: CPU-made and reproducible.
  kind   abs: the box is on u_t, its rows are the nominal actuated positions plus the offsets below;
         rel: the box is on u_t - u_{t-1}, its rows are the offsets.
  shape  every width is drawn per step and per component in w U(0.3, 2), independently for the two sides.
         ragged     all finite
         one_sided  per component one side infinite at every step: the side the unconstrained first tail leans on
                    keeps its bound, so the finite side binds
         gaps       each entry of lo and, independently, of hi infinite with probability 0.4; one whole step and
                    (m > 1) one whole component free on both sides
         pinned     30 % of the entries have hi == lo
         offzero    lo = -w r + 0.5 w, hi = lo + 0.6 w: the box mostly excludes the nominal (abs) or zero (rel)
         none       no rows at all (null pointers);  allinf: rows that are infinite throughout
  T      11 and 12 (the tiles kernel sweeps two steps per loop trip); 1 and 2 with `ragged`.
The bound rows of a case are seeded by its id and, where the first draw does not meet the conditions of
tests/test_ctrlbox_cases_cpu.py, by the SEED table.

tail_reference is the certificate the device is held to, tail by tail: the tail QP in its ORIGINAL statement
(tv_lqr.py, position-controlled branch) condensed to a dense H z + g by unrolling the dynamics -- it goes through
neither quasistatic_ctrl_problem nor ctrlbox_backward -- and a candidate optimum that is accepted only when it meets
the box, is stationary on its free entries and has multipliers of the right sign at lo and at hi.  mutated_rows are
the three row-handling errors a case has to be able to see.
"""
import functools

import numpy as np

from oracle import irs_oracle as orc

_HAND, _BOX = orc.PlanarHandOracle, orc.BoxPivotOracle

def _bob_goal(T):
    """Box-on-box: the box is wanted 0.5 further out over the first half of the horizon and 0.08 back from its start
    over the second.  The pusher can only push: the descent leans on its upper bounds first and on its lower bounds
    after, so this one-control model binds on both sides too."""
    g = np.zeros((T + 1, 2))
    g[:, 1] = np.where(np.arange(T + 1) <= T // 2, 0.5, -0.08)
    return g


# model -> (oracle system, x0, diagonal of Q, goal offset: one row, or a function of T that gives (T + 1, n) rows)
MODELS = {
    "hand": (lambda: orc.PlanarHandOracle(0.1),
             _HAND.pack([0.0, 0.35, 0.0], [-np.pi / 4, -np.pi / 4], [np.pi / 4, np.pi / 4]),
             _HAND.pack([1e-3, 1e-3, 10.0], [1e-3, 1e-3], [1e-3, 1e-3]), _HAND.pack([0.3, -0.1, 0.5], [0, 0], [0, 0])),
    "pivot": (lambda: orc.BoxPivotOracle(0.1), _BOX.pack([0.0, 0.5, 0.0], [-0.62, 0.3]),
              _BOX.pack([5, 5, 50], [0, 0]), _BOX.pack([0.5, 0.0, -0.4], [0, 0])),
    "push": (lambda: orc.BoxPushOracle(0.1), _BOX.pack([0.0, 0.5, 0.0], [0.0, -0.2]),
             _BOX.pack([5, 5, 50], [0, 0]), _BOX.pack([0.5, 0.5, -0.4], [0, 0])),
    "bob": (lambda: orc.BoxOnBoxOracle(0.1, 1.0, 100.0), np.array([0.9, 1.0]), np.array([0.0, 10.0]), _bob_goal),
}
KINDS = ("abs", "rel")
BOUNDED = ("ragged", "one_sided", "gaps", "pinned", "offzero")
SHAPES = BOUNDED + ("none", "allinf")
T_MAIN, T_SHORT = (11, 12), (1, 2)
WIDTH = {"abs": 0.05, "rel": 0.03}            # the trust region and the rate limit of the suite's descents
RES_TOL = 1e-9                                # the certificate: residuals relative to max |g|
AT_TOL = 1e-12                                # an entry is AT a bound within this (the candidates sit on it exactly)
# (model, kind, shape, T) -> last word of the seed of the bound rows where it is not 0: the first one at which the
# case meets the conditions of tests/test_ctrlbox_cases_cpu.py (which holds every case to them)
SEED = {("hand", "rel", "gaps", 12): 1, ("pivot", "rel", "gaps", 11): 1}


def cid_of(model, kind, shape, T):
    return "%s-%s-%s-T%d" % (model, kind, shape, T)


def _case_list():
    out = []
    for model in MODELS:
        for kind in KINDS:
            out += [(model, kind, s, T) for s in BOUNDED for T in T_MAIN]
            out += [(model, kind, "allinf", T) for T in T_MAIN]
            out += [(model, kind, "ragged", T) for T in T_SHORT]
        out += [(model, "abs", "none", T) for T in T_MAIN]    # null pointers have no kind: the kernels run them as abs
    return out


CASES = {cid_of(*c): c for c in _case_list()}


# ------------------------------------------------------------------------------------------------ problem data
@functools.lru_cache(maxsize=None)
def problem(model, T):
    """Seeded data of one model and horizon: x0, the nominal (u_trj, x_trj), (At, Bt, ct), Q, Qd, R, xd, idx."""
    make, x0, q, goal = MODELS[model]
    sys_o = make()
    idx = np.asarray(sys_o.indices_u_into_x)
    m = len(idx)
    rng = np.random.default_rng([list(MODELS).index(model), T, 7])
    u_trj = np.tile(x0[idx], (T, 1)) + 0.02 * rng.normal(size=(T, m)).cumsum(axis=0)
    x_trj = orc.rollout(sys_o, x0, u_trj)
    du = 0.1 * rng.normal(size=(T, 300, m))
    At, Bt, ct = orc.zero_order_B_decoupled(sys_o, x_trj, u_trj, du)
    return dict(model=model, T=T, n=len(x0), m=m, idx=idx, x0=np.array(x0, float), u_trj=u_trj, x_trj=x_trj, At=At,
                Bt=Bt, ct=ct, Q=np.diag(q), Qd=np.diag(10.0 * q), R=5.0 * np.eye(m),
                xd=x0 + (goal(T) if callable(goal) else np.tile(goal, (T + 1, 1))))


def system(model):
    """A fresh oracle system of the model (its contact step is the dynamics of the oracle loop)."""
    return MODELS[model][0]()


# ------------------------------------------------------------------------------------------------ the certificate
def condensed(p, kind, t, x_t, lo, hi):
    """The tail QP t .. T-1 from x_t in the original statement, condensed: cost(z) = z'H z + 2 g'z + c0 over the
    stacked bounded quantity z ((T-t) m: u for abs, du for rel), with lo <= z <= hi.  States by x+ = A x + B u + c,
    stage cost (x - xd)'Q(x - xd) + du'R du with du_t = u_t - x_t[idx], terminal Qd.  Returns H, g, c0, the stacked
    rows and the affine map z -> u (S, u0)."""
    T, n, m, idx = p["T"], p["n"], p["m"], p["idx"]
    N = T - t
    w = np.asarray(x_t, float)[idx]
    # u = S z + u0
    if kind == "abs":
        S, u0 = np.eye(N * m), np.zeros(N * m)
    else:
        S, u0 = np.kron(np.tril(np.ones((N, N))), np.eye(m)), np.tile(w, N)
    # du = D u - d0
    D = np.eye(N * m) - np.kron(np.eye(N, k=-1), np.eye(m))
    d0 = np.concatenate([w, np.zeros((N - 1) * m)])
    # x_{t+k+1} = F_k u + f_k
    F, f = np.zeros((N + 1, n, N * m)), np.zeros((N + 1, n))
    f[0] = x_t
    for k in range(N):
        A, B, c = p["At"][t + k], p["Bt"][t + k], p["ct"][t + k]
        F[k + 1] = A @ F[k]
        F[k + 1][:, k * m:(k + 1) * m] += B
        f[k + 1] = A @ f[k] + c
    Hu, gu, c0 = np.zeros((N * m, N * m)), np.zeros(N * m), 0.0
    for k in range(N + 1):
        W = p["Qd"] if k == N else p["Q"]
        e = f[k] - p["xd"][t + k]
        Hu += F[k].T @ W @ F[k]
        gu += F[k].T @ (W @ e)
        c0 += e @ W @ e
    Rb = np.kron(np.eye(N), p["R"])
    Hu += D.T @ Rb @ D
    gu -= D.T @ (Rb @ d0)
    c0 += d0 @ Rb @ d0
    # substitute u = S z + u0
    H = S.T @ Hu @ S
    g = S.T @ (Hu @ u0 + gu)
    c0 += u0 @ Hu @ u0 + 2.0 * gu @ u0
    H = 0.5 * (H + H.T)
    return dict(H=H, g=g, c0=c0, lo=np.asarray(lo[t:], float).reshape(-1), hi=np.asarray(hi[t:], float).reshape(-1),
                S=S, u0=u0, N=N, m=m)


def condensed_cost(q, z):
    return float(z @ q["H"] @ z + 2.0 * q["g"] @ z + q["c0"])


def certificate(q, z):
    """The solver-independent optimality conditions of z on a condensed QP: (box violation, stationarity on the free
    entries, wrong-signed multiplier at lo, at hi), the last three relative to max |g|; and per entry the side it sits
    on: (at lo, at hi) as masks -- an entry with lo == hi is at both and exempt from the sign condition -- and as a
    sign (-1 lo, +1 hi, 0 free or lo == hi); and its strict-complementarity margin (free: the distance to the nearer
    bound; at a bound: |multiplier| / max |g|; lo == hi: 0, its side means nothing)."""
    lo, hi = q["lo"], q["hi"]
    grad = q["H"] @ z + q["g"]                     # half the gradient: >= 0 at lo, <= 0 at hi, 0 where free
    scale = max(np.abs(q["g"]).max(), 1e-300)
    with np.errstate(invalid="ignore"):
        at_lo = np.isfinite(lo) & (np.abs(z - lo) <= AT_TOL * (1.0 + np.abs(lo)))
        at_hi = np.isfinite(hi) & (np.abs(z - hi) <= AT_TOL * (1.0 + np.abs(hi)))
    pinned = at_lo & at_hi
    free = ~at_lo & ~at_hi
    r_box = max(float(np.maximum(lo - z, 0.0).max()), float(np.maximum(z - hi, 0.0).max()))
    r_stat = float(np.abs(grad[free]).max() / scale) if free.any() else 0.0
    r_lo = float(np.maximum(-grad[at_lo & ~pinned], 0.0).max() / scale) if (at_lo & ~pinned).any() else 0.0
    r_hi = float(np.maximum(grad[at_hi & ~pinned], 0.0).max() / scale) if (at_hi & ~pinned).any() else 0.0
    side = np.where(pinned, 0, np.where(at_lo, -1, np.where(at_hi, 1, 0)))
    margin = np.where(free, np.minimum(z - lo, hi - z), np.abs(grad) / scale)
    margin = np.where(pinned, 0.0, margin)
    return (r_box, r_stat, r_lo, r_hi), (at_lo, at_hi), side, margin


def _candidate(case, t, x_t):
    """orc.ctrlbox_solve, cold, on the tail: any method may propose; the certificate decides."""
    p = case
    prob = orc.quasistatic_ctrl_problem(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["xd"], case["kind"])
    W = orc.ctrlbox_workspace(prob)
    T, m = p["T"], p["m"]
    act, u = np.zeros((T, m), dtype=int), np.zeros((T, m))
    s_t = np.concatenate([x_t, np.asarray(x_t)[p["idx"]]])
    _, u, _, st, _ = orc.ctrlbox_solve(prob, s_t, t, case["lo"], case["hi"], u, act, W, T, tol=1e-12)
    return np.clip(u[t:], case["lo"][t:], case["hi"][t:]).reshape(-1), st


def tail_reference(case, t, x_t):
    """The optimum of tail t .. T-1 of the case started from s = [x_t; x_t[idx]], certified: dict(u0 = the first
    control (clipped to its row; rel: plus x_t[idx]), at_lo / at_hi = which first-row entries sit at a finite bound,
    margin = the smallest strict-complementarity margin of that row, res = the certificate's residuals, ok = all of
    them below RES_TOL, z / side / margins = the whole tail ((T-t, m)), converged = the candidate's solver finished)."""
    x_t = np.asarray(x_t, float)
    m = case["m"]
    q = condensed(case, case["kind"], t, x_t, case["lo"], case["hi"])
    z, st = _candidate(case, t, x_t)
    res, (at_lo, at_hi), side, margin = certificate(q, z)
    row = np.clip(z[:m], case["lo"][t], case["hi"][t])
    u0 = row if case["kind"] == "abs" else x_t[case["idx"]] + row
    return dict(u0=u0, at_lo=at_lo[:m], at_hi=at_hi[:m], margin=float(margin[:m].min()), res=res,
                ok=max(res) < RES_TOL, z=z.reshape(-1, m), side=side.reshape(-1, m), margins=margin.reshape(-1, m),
                converged=st[1] >= 0, q=q)


# ------------------------------------------------------------------------------------------------ bound rows
def _draw(rng, T, m, w):
    """Offsets (lo < 0 < hi) of independent widths w U(0.3, 2) per step, component and side."""
    return -w * rng.uniform(0.3, 2.0, size=(T, m)), w * rng.uniform(0.3, 2.0, size=(T, m))


def _unconstrained_lean(p, kind, off_lo, off_hi):
    """Per entry, by how much the unconstrained first tail (in the bounded quantity, relative to the row centre)
    leaves the ragged box: (below lo, above hi), each >= 0."""
    T, m = p["T"], p["m"]
    centre = p["x_trj"][:-1, p["idx"]] if kind == "abs" else np.zeros((T, m))
    q = condensed(p, kind, 0, p["x0"], np.full((T, m), -np.inf), np.full((T, m), np.inf))
    z = np.linalg.solve(q["H"], -q["g"]).reshape(T, m) - centre
    return np.maximum(off_lo - z, 0.0), np.maximum(z - off_hi, 0.0)


def offsets(model, kind, shape, T):
    """(off_lo, off_hi) (T, m) of a case, +-inf where free: the rows are centre + offsets, centre = the nominal
    actuated positions x_trj[:-1, idx] (abs) or 0 (rel).  None, None for `none`."""
    p = problem(model, T)
    m, w = p["m"], WIDTH[kind]
    rng = np.random.default_rng([list(MODELS).index(model), KINDS.index(kind), SHAPES.index(shape), T,
                                 SEED.get((model, kind, shape, T), 0)])
    lo, hi = _draw(rng, T, m, w)
    ragged_lo, ragged_hi = lo.copy(), hi.copy()
    inf = np.inf
    if shape == "none":
        return None, None
    if shape == "allinf":
        return np.full((T, m), -inf), np.full((T, m), inf)
    if shape == "one_sided":
        below, above = _unconstrained_lean(p, kind, lo, hi)
        keep_hi = above.sum(axis=0) >= below.sum(axis=0)            # per component
        lo[:, keep_hi], hi[:, ~keep_hi] = -inf, inf
    if shape == "gaps":
        lo[rng.random((T, m)) < 0.4] = -inf
        hi[rng.random((T, m)) < 0.4] = inf
        lo[T // 2], hi[T // 2] = -inf, inf                          # a whole step free
        if m > 1:
            below, above = _unconstrained_lean(p, kind, ragged_lo, ragged_hi)
            j = int(np.argmin((below + above).sum(axis=0)))         # the component that leans least: nothing lost
            lo[:, j], hi[:, j] = -inf, inf
    if shape == "pinned":
        pin = rng.random((T, m)) < 0.3
        if not pin[0].any():
            pin[0, 0] = True                                        # a pinned entry in the first row of the first tail
        hi[pin] = lo[pin]
    if shape == "offzero":
        r = rng.uniform(0.3, 2.0, size=(T, m))
        lo = -w * r + 0.5 * w
        hi = lo + 0.6 * w
    return lo, hi


def rows_from_offsets(p, kind, off_lo, off_hi, x_trj=None):
    """Absolute rows of the offsets around a nominal trajectory (default: the case's own)."""
    if off_lo is None:
        return None, None
    if kind == "rel":
        return off_lo.copy(), off_hi.copy()
    centre = (p["x_trj"] if x_trj is None else x_trj)[:-1, p["idx"]]
    return centre + off_lo, centre + off_hi


@functools.lru_cache(maxsize=None)
def case(cid):
    """The full problem of a case id: problem(model, T) plus kind, shape, the offsets, and lo / hi (T, m) rows as the
    oracle reads them (infinite throughout for `none`); `null` says the device gets no row pointers."""
    model, kind, shape, T = CASES[cid]
    c = dict(problem(model, T))
    off_lo, off_hi = offsets(model, kind, shape, T)
    lo, hi = rows_from_offsets(c, kind, off_lo, off_hi)
    null = lo is None
    if null:
        lo, hi = np.full((T, c["m"]), -np.inf), np.full((T, c["m"]), np.inf)
    c.update(id=cid, kind=kind, shape=shape, off_lo=off_lo, off_hi=off_hi, lo=lo, hi=hi, null=null)
    return c


def with_rows(c, lo, hi, **other):
    """The case with other rows (and other data: At=..., x_trj=...)."""
    return dict(c, lo=lo, hi=hi, **other)


def binds(c):
    """Whether the case is built to bind (none / allinf cannot)."""
    return c["shape"] in BOUNDED


# ------------------------------------------------------------------------------------------------ the oracle loop
def oracle_descent(c, rows=None, sys_o=None):
    """orc.local_descent_quasistatic_as on the case (with `rows` = (lo, hi) in place of its own): x_new, u_new,
    stats."""
    lo, hi = (c["lo"], c["hi"]) if rows is None else rows
    sys_o = system(c["model"]) if sys_o is None else sys_o
    return orc.local_descent_quasistatic_as(sys_o, c["At"], c["Bt"], c["ct"], c["Q"], c["Qd"], c["R"], c["x0"],
                                            c["xd"], lo, hi, c["kind"])


def certify_trajectory(c, x_new, u_new):
    """Every tail of a closed-loop descent (x_new, u_new) against tail_reference started from x_new[t]: the certified
    first controls (T, m), which of them sit at lo / at hi (T, m), the per-tail references, and the worst residual."""
    T = c["T"]
    refs = [tail_reference(c, t, x_new[t]) for t in range(T)]
    return dict(u=np.stack([r["u0"] for r in refs]), at_lo=np.stack([r["at_lo"] for r in refs]),
                at_hi=np.stack([r["at_hi"] for r in refs]), refs=refs, ok=all(r["ok"] for r in refs),
                converged=all(r["converged"] for r in refs), worst=max(max(r["res"]) for r in refs))


# ------------------------------------------------------------------------------------------------ mutations
MUTATIONS = ("shift", "row0", "swapcol")


def mutated_rows(c, how):
    """The row-handling errors a case has to be able to see, as (lo, hi) rows; None where the error changes nothing
    (one row: nothing to shift or broadcast; one component: nothing to reverse).
      shift    rows read one step late: step t uses row t + 1 (the last row stays)
      row0     row 0 at every step
      swapcol  the components reversed"""
    lo, hi = c["lo"], c["hi"]
    if how == "shift":
        out = np.vstack([lo[1:], lo[-1:]]), np.vstack([hi[1:], hi[-1:]])
    elif how == "row0":
        out = np.tile(lo[0], (lo.shape[0], 1)), np.tile(hi[0], (hi.shape[0], 1))
    elif how == "swapcol":
        out = lo[:, ::-1].copy(), hi[:, ::-1].copy()
    else:
        raise ValueError(how)
    same = np.array_equal(out[0], lo) and np.array_equal(out[1], hi)
    return None if same else out
