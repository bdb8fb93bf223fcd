"""Extended-precision reference of the TV-LQR backward pass and of the closed-loop rollout on the linear
model, and the dense-weight inputs the conformance tests feed to the device kernels.

Arithmetic is np.longdouble (64-bit mantissa on x86-64, eps ~1.1e-19; where the platform's long double is
the f64 the answers are still right, the conditioning checks of tests/test_tvlqr_reference_cpu.py then
compare f64 with f64).  LAPACK has no long-double path, so the small SPD systems
H = alpha R + B'PB are solved here by a Cholesky factorisation written out below; NumPy's matrix product
falls back to plain loops for this type, which is what is wanted.

The weights.  The cost (x - xd)'Q(x - xd) depends only on the symmetric part of Q: x'Sx = 0 for every
antisymmetric S.  Drake's AddQuadraticErrorCost / AddQuadraticCost, with which the reference builds its QP
(irs_lqr/tv_lqr.py:107-130), store the symmetric part.  The recursion P <- Q + A'P(A + BK) however is NOT
invariant: fed an unsymmetric Q it carries an unsymmetric P, and (PB)'A differs from B'PA.  So a weight that
is not symmetric (an upper triangle, say) is a valid input whose answer is that of (Q + Q')/2, and this
reference takes the symmetric part of Q, Qd and R on entry.  (oracle/irs_oracle.py:tvlqr_riccati does not;
hand it symmetric weights.)
"""
import functools

import numpy as np

LD = np.longdouble


def sym(M):
    """Symmetric part, in extended precision."""
    M = np.asarray(M, dtype=LD)
    return 0.5 * (M + M.T)


def cholesky(H):
    """Lower-triangular L with L L' = H (H symmetric positive definite); raises np.linalg.LinAlgError with the
    1-based pivot otherwise."""
    H = np.asarray(H, dtype=LD)
    m = H.shape[0]
    L = np.zeros((m, m), dtype=LD)
    for j in range(m):
        d = H[j, j] - L[j, :j].dot(L[j, :j])
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite at pivot %d" % (j + 1))
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, m):
            L[i, j] = (H[i, j] - L[i, :j].dot(L[j, :j])) / L[j, j]
    return L


def cho_solve(L, B):
    """Solve (L L') X = B for a matrix or vector B."""
    B = np.asarray(B, dtype=LD)
    vec = B.ndim == 1
    Y = np.array(B.reshape(B.shape[0], -1), dtype=LD, copy=True)
    m = L.shape[0]
    for i in range(m):
        Y[i] = (Y[i] - L[i, :i].dot(Y[:i])) / L[i, i]
    for i in range(m - 1, -1, -1):
        Y[i] = (Y[i] - L[i + 1:, i].dot(Y[i + 1:])) / L[i, i]
    return Y[:, 0] if vec else Y


def tvlqr_riccati(At, Bt, ct, Q, Qd, R, xd_trj, alpha_R=0.5):
    """Backward pass of the QP of oracle/irs_oracle.py:solve_tvlqr_qp,
        H = alpha_R R + B'PB,  K = -H^-1 B'PA,  k = -H^-1 B'(Pc + p),
        P <- Q + A'P(A + BK),  p <- -Q xd_t + (A + BK)'(Pc + p),     P_T = Qd, p_T = -Qd xd_T,
    on the symmetric parts of Q, Qd, R.  Returns K (T,m,n), k (T,m) as longdouble arrays."""
    At, Bt, ct, xd = (np.asarray(a, dtype=LD) for a in (At, Bt, ct, xd_trj))
    Q, Qd, R = sym(Q), sym(Qd), sym(R)
    T, n, m = At.shape[0], Q.shape[0], R.shape[0]
    K = np.zeros((T, m, n), dtype=LD)
    k = np.zeros((T, m), dtype=LD)
    P = Qd.copy()
    p = -Qd.dot(xd[T])
    aR = LD(alpha_R) * R
    for t in range(T - 1, -1, -1):
        A, B, c = At[t], Bt[t], ct[t]
        PB = P.dot(B)
        L = cholesky(aR + B.T.dot(PB))
        q = P.dot(c) + p
        K[t] = -cho_solve(L, PB.T.dot(A))
        k[t] = -cho_solve(L, B.T.dot(q))
        Acl = A + B.dot(K[t])
        P = sym(Q + A.T.dot(P).dot(Acl))
        p = -Q.dot(xd[t]) + Acl.T.dot(q)
    return K, k


def pivot_trace(At, Bt, Q, Qd, R, alpha_R=0.5, cross=None, half_rho=0.0, pen_x=None, pen_u=None):
    """The control Hessians of the backward sweep, in extended precision, up to the first one that is not positive
    definite -- the reference of the descents' `info[0]` (include/irs_hip.h, rule V1).

    Stage cost z'Q^z + 2 z'S v + v'R^v, terminal z'Qd^z (the linear terms do not enter a Hessian):
        H_t = R^ + B_t'P_{t+1}B_t,   G_t = S' + B_t'P_{t+1}A_t,   P_t = Q^ + A_t'P_{t+1}A_t - G_t'H_t^-1 G_t,   P_T = Qd^.
      cross     S (n,m), None = 0: the position-controlled QP written on the absolute command (position_controlled_form)
      half_rho, pen_x (n), pen_u (m): the ADMM's penalised weights as csrc/boxqp_factor.inc states them,
                Q^ = sym(Q) + rho/2 Mx,  Qd^ = sym(Qd) + rho/2 Mx,  R^ = alpha_R sym(R) + rho/2 Mu,
                Mx / Mu = diag of the 0/1 masks of the finitely bounded components (None = no penalty).
    Returns (t_bad, H): H[t] = H_t (m,m) for t = T-1 down to t_bad, where the Cholesky factorisation of H_{t_bad}
    fails and the sweep stops -- the Hessians are those of the P computed from the steps after t_bad; t_bad = None
    (and H holds every step) when all of them are positive definite."""
    At, Bt = np.asarray(At, dtype=LD), np.asarray(Bt, dtype=LD)
    T, n, m = At.shape[0], At.shape[1], Bt.shape[2]
    Mx = np.diag(np.asarray(pen_x if pen_x is not None else np.zeros(n), dtype=LD)) * LD(half_rho)
    Mu = np.diag(np.asarray(pen_u if pen_u is not None else np.zeros(m), dtype=LD)) * LD(half_rho)
    Qh, Rh = sym(Q) + Mx, LD(alpha_R) * sym(R) + Mu
    S = np.zeros((n, m), dtype=LD) if cross is None else np.asarray(cross, dtype=LD)
    P = sym(Qd) + Mx
    H = {}
    for t in range(T - 1, -1, -1):
        A, B = At[t], Bt[t]
        PB = P.dot(B)
        H[t] = sym(Rh + B.T.dot(PB))
        try:
            L = cholesky(H[t])
        except np.linalg.LinAlgError:
            return t, H
        G = S.T + PB.T.dot(A)
        P = sym(Qh + A.T.dot(P).dot(A) - G.T.dot(cho_solve(L, G)))
    return None, H


def position_controlled_form(At, Bt, Q, Qd, R, control="du"):
    """The QP of the position-controlled descents (irs_quasistatic_box_descent; irs_lqr/tv_lqr.py:96-108: input cost
    du_t'R du_t, du_t = u_t - u_{t-1}) on the augmented state z = [x; u_prev], as pivot_trace takes it.  Two spellings
    of the same problem, whose control Hessians agree (u = u_prev + du is a shift of the control):
      "du"   control du: A~ = [A B; 0 I], B~ = [B; I], cost x'Qx + du'R du            (the ADMM, the rate-limited boxes)
      "abs"  control u:  A~ = [A 0; 0 0], B~ = [B; I], cost x'Qx + (u - w)'R(u - w)   (the trust-region boxes)
             = z'diag(Q, R)z - 2 w'R u + u'Ru: a stage cross term S = [0; -R].
    Returns dict(At, Bt, Q, Qd, R, cross) for pivot_trace(..., alpha_R=1)."""
    At, Bt = np.asarray(At, dtype=LD), np.asarray(Bt, dtype=LD)
    T, n, m = At.shape[0], At.shape[1], Bt.shape[2]
    Q, Qd, R = sym(Q), sym(Qd), sym(R)
    Aa = np.zeros((T, n + m, n + m), dtype=LD)
    Ba = np.zeros((T, n + m, m), dtype=LD)
    Aa[:, :n, :n] = At
    Ba[:, :n, :] = Bt
    Ba[:, n:, :] = np.eye(m, dtype=LD)
    Qa = np.zeros((n + m, n + m), dtype=LD)
    Qa[:n, :n] = Q
    Qda = np.zeros((n + m, n + m), dtype=LD)
    Qda[:n, :n] = Qd
    cross = None
    if control == "du":
        Aa[:, :n, n:] = Bt
        Aa[:, n:, n:] = np.eye(m, dtype=LD)
    elif control == "abs":
        Qa[n:, n:] = R
        cross = np.zeros((n + m, m), dtype=LD)
        cross[n:, :] = -R
    else:
        raise ValueError(control)
    return dict(At=Aa, Bt=Ba, Q=Qa, Qd=Qda, R=R, cross=cross)


def definiteness_margin(H):
    """lambda_min(H) / max|H|: f64 eigvalsh of the extended-precision H (the margins asked of it are ten decades above
    f64 rounding)."""
    H = np.asarray(H, dtype=float)
    return float(np.linalg.eigvalsh(0.5 * (H + H.T)).min() / np.abs(H).max())


def linear_rollout(At, Bt, ct, K, k, x0):
    """u_t = K_t x_t + k_t, x_{t+1} = A_t x_t + B_t u_t + c_t in extended precision: x (T+1,n), u (T,m)."""
    At, Bt, ct, K, k = (np.asarray(a, dtype=LD) for a in (At, Bt, ct, K, k))
    T, m, n = K.shape
    x = np.zeros((T + 1, n), dtype=LD)
    u = np.zeros((T, m), dtype=LD)
    x[0] = np.asarray(x0, dtype=LD)
    for t in range(T):
        u[t] = K[t].dot(x[t]) + k[t]
        x[t + 1] = At[t].dot(x[t]) + Bt[t].dot(u[t]) + ct[t]
    return x, u


def solve_tvlqr(At, Bt, ct, Q, Qd, R, x0, xd_trj, alpha_R=0.5):
    """The plan of the unconstrained QP: backward pass, then the rollout of its policy on the linear model."""
    K, k = tvlqr_riccati(At, Bt, ct, Q, Qd, R, xd_trj, alpha_R)
    return linear_rollout(At, Bt, ct, K, k, x0)


# ----------------------------------------------------------------------------------------------------------
# Conformance inputs: what tests/test_tvlqr_reference_cpu.py qualifies and tests/test_tvlqr_dense_gpu.py runs
# ----------------------------------------------------------------------------------------------------------
# The device tolerance on everything computed in f64 (tests/test_gpu_parity.py); the inputs below are admitted
# only if the f64 oracle stays within 1/100 of it of the extended-precision answer.
GPU_TOL = dict(rtol=1e-8, atol=1e-9)

# irs_tvlqr_riccati dispatches on (n, m) and, for the matrix-core sizes, on (T + 1) n <= 4096 (csrc/tvlqr.hip,
# riccati_backward_any): every implementation, and both sides of that switch.  (n, m, T, implementation)
RICCATI_CASES = (
    (2, 1, 1, "registers"), (2, 1, 2, "registers"), (2, 1, 30, "registers"),
    (5, 2, 818, "mfma"), (5, 2, 819, "lds"),
    (6, 2, 681, "mfma"), (6, 2, 682, "lds"),
    (7, 4, 584, "mfma"), (7, 4, 585, "lds"),
    (12, 4, 1, "mfma"), (12, 4, 340, "mfma"), (12, 4, 341, "lds"),
    (1, 1, 1, "generic"), (3, 2, 17, "generic"), (4, 2, 50, "generic"), (15, 4, 30, "generic"),
    (16, 4, 23, "generic"), (3, 16, 9, "generic"), (32, 16, 12, "generic"),
)
FAMILIES = ("spd", "psd_null", "scaled")
GRID = 2.0 ** -30


def on_grid(M):
    """Entries rounded to multiples of 2^-30.  All weights here are below 2^11 in magnitude, so s + k, s - k and
    (s + k) + (s - k) are exact in f64 for grid values s, k: the symmetric part of `W + skew` IS W, bit for bit,
    and a comparison of the two answers measures what a kernel does with the skew part and nothing else."""
    return np.round(np.asarray(M, float) / GRID) * GRID


def _rotation(rng, n):
    q, r = np.linalg.qr(rng.normal(size=(n, n)))
    return q * np.sign(np.diag(r))


def _rotated(rng, d):
    V = _rotation(rng, len(d))
    W = (V * d).dot(V.T)
    return 0.5 * (W + W.T)


def weight(rng, n, family, ridge, definite=False, decades=3):
    """One dense symmetric n x n weight on the grid.
      spd       G G'/n + ridge I
      psd_null  V diag(d) V', V a random rotation, d in [0.5, 2] with max(1, n // 3) entries zero (n >= 2):
                the quadrotor's velocity-free Q, no longer axis-aligned.  `definite` (the control weight R, which
                has to be definite for the QP to have one solution) keeps every d positive
      scaled    V diag(d) V', d log-spaced over 10^-decades .. 10^decades (n = 1: d = 1)"""
    if family == "spd":
        G = rng.normal(size=(n, n))
        W = G.dot(G.T) / n + ridge * np.eye(n)
    elif family == "psd_null":
        d = rng.uniform(0.5, 2.0, size=n)
        if n >= 2 and not definite:
            d[rng.permutation(n)[:max(1, n // 3)]] = 0.0
        W = _rotated(rng, d)
    elif family == "scaled":
        d = np.logspace(-decades, decades, n) if n > 1 else np.ones(1)
        W = _rotated(rng, rng.permutation(d))
    else:
        raise ValueError(family)
    return on_grid(0.5 * (W + W.T))


def weights(rng, n, m, family):
    """(Q, Qd, R) of one family.  Q and Qd may be singular (psd_null); R is always definite.  With more controls
    than states B'PB has rank <= n, so m - n directions of H = alpha R + B'PB see R alone and cond(H) >= the
    spread of R there: the scaled R then spans 1e-1 .. 1e1 instead of 1e-3 .. 1e3, which keeps the f64 oracle
    itself within 1/100 of the device tolerance (the admission rule of these inputs)."""
    return (weight(rng, n, family, 0.1), weight(rng, n, family, 0.5),
            weight(rng, m, family, 0.2, definite=True, decades=3 if m <= n else 1))


def skew_variants(W, rng, a=0.3):
    """Unsymmetric spellings of the symmetric grid matrix W whose symmetric part is exactly W:
    W + a (S - S') with S standard normal (on the grid), and the upper triangle triu(2 W) - diag(W)."""
    n = W.shape[0]
    S = on_grid(a * rng.normal(size=(n, n)))
    return {"skew": W + (S - S.T), "triu": np.triu(2.0 * W) - np.diag(np.diag(W))}


@functools.lru_cache(maxsize=None)
def riccati_problem(n, m, T, family):
    """The TV-LQR problem of one conformance case, from a seed fixed by the case:
    A_t = I + 0.1 N(0,1), B_t, xd_t standard normal, c_t = 0.1 N(0,1), x0 standard normal."""
    rng = np.random.default_rng([n, m, T, FAMILIES.index(family)])
    At = np.eye(n) + 0.1 * rng.normal(size=(T, n, n))
    Bt = rng.normal(size=(T, n, m))
    ct = 0.1 * rng.normal(size=(T, n))
    xd = rng.normal(size=(T + 1, n))
    x0 = rng.normal(size=n)
    Q, Qd, R = weights(rng, n, m, family)
    var = {name: (skew_variants(Q, rng)[name], skew_variants(Qd, rng)[name], skew_variants(R, rng)[name])
           for name in ("skew", "triu")}
    return dict(At=At, Bt=Bt, ct=ct, xd=xd, x0=x0, Q=Q, Qd=Qd, R=R, unsym=var)


@functools.lru_cache(maxsize=None)
def riccati_reference(n, m, T, family):
    """(K, k) of riccati_problem in extended precision."""
    p = riccati_problem(n, m, T, family)
    return tvlqr_riccati(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["xd"], alpha_R=0.5)


def within(got, want, frac=1.0, rtol=GPU_TOL["rtol"], atol=GPU_TOL["atol"]):
    """max over entries of |got - want| / (frac (atol + rtol |want|)): <= 1 passes.  Evaluated in extended
    precision so that the reference's extra digits count."""
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    return float(np.max(np.abs(got - want) / (LD(frac) * (LD(atol) + LD(rtol) * np.abs(want)))))


# the device models whose descent, rollout and cost kernels take dense weights in the GPU tests: (name, h, T).
# pendulum: the register rollout (n <= 4); the others: the LDS-staged one; quadrotor T = 341: the fused descent
# kernel with its Riccati pass beyond the matrix-core horizon
MODEL_CASES = (("pendulum", 0.05, 30), ("bicycle", 0.1, 25), ("three_cart", 0.05, 25), ("quadrotor", 0.05, 20),
               ("quadrotor", 0.05, 341))
_MODEL_START = {"pendulum": ([0.0, 0.0], [0.1]), "bicycle": ([0.0] * 5, [0.1, 0.0]),
                "three_cart": ([0.0, 1.0, 2.0, 0.0, 0.0, 0.0], [0.1, -0.1]), "quadrotor": ([0.0] * 12, [2.0] * 4)}


@functools.lru_cache(maxsize=None)
def model_problem(name, h, T):
    """One descent problem of a device model with dense SPD weights: the example's start and nominal input, the
    exact linearisation along its rollout, and a goal trajectory a little off the nominal one (so that the closed
    loop on the true dynamics stays where the linearisation holds, at any horizon)."""
    from oracle import irs_oracle as orc
    sys_o = orc.SYSTEMS[name](h)
    n, m = sys_o.dim_x, sys_o.dim_u
    rng = np.random.default_rng([sorted(orc.SYSTEMS).index(name), T])
    x0, u0 = (np.array(v, float) for v in _MODEL_START[name])
    u_trj = np.tile(u0, (T, 1))
    x_trj = orc.rollout(sys_o, x0, u_trj)
    At, Bt, ct = orc.exact_TV(sys_o, x_trj, u_trj)
    xd = x_trj + 0.05 * rng.normal(size=n) + 0.02 * np.sin(0.3 * np.arange(T + 1))[:, None] * rng.normal(size=n)
    Q, Qd, R = weights(rng, n, m, "spd")
    var = {v: (skew_variants(Q, rng)[v], skew_variants(Qd, rng)[v], skew_variants(R, rng)[v]) for v in ("skew", "triu")}
    return dict(sys_o=sys_o, x0=x0, u_trj=u_trj, x_trj=x_trj, At=At, Bt=Bt, ct=ct, xd=xd, Q=Q, Qd=Qd, R=R, unsym=var)


# candidates of the CEM cost kernels: (name, h, T, std of the input noise around the nominal input)
CEM_CASES = (("pendulum", 0.05, 30, 0.05), ("quadrotor", 0.05, 20, 0.005))


@functools.lru_cache(maxsize=None)
def cem_candidates(name, h, T, std, B=64):
    """B open-loop input sequences around the nominal input of model_problem, and the oracle's cost of each.
    An open-loop rollout has no feedback to absorb a rounding error: the quadrotor's differential thrust acts on
    an inertia of ~1e-3, so noise of 0.05 per rotor tumbles some candidates through the Euler-angle singularity
    within a second (costs of 1e8 and beyond, sensitive to the last bit of the dynamics), which says nothing
    about how a kernel reads Q.  Its noise is therefore 0.005 (attitude stays within ~0.1 rad);
    tests/test_tvlqr_reference_cpu.py admits the candidates by the oracle's own sensitivity."""
    p = model_problem(name, h, T)
    rng = np.random.default_rng([B, T])
    cand = p["u_trj"] + std * rng.normal(size=(B, T, p["u_trj"].shape[1]))
    return cand, open_loop_costs(p, cand)


def open_loop_costs(p, cand):
    from oracle import irs_oracle as orc
    return np.array([orc.evaluate_cost(orc.rollout(p["sys_o"], p["x0"], u), u, p["xd"], p["Q"], p["R"]) for u in cand])
