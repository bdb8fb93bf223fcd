"""NumPy twin (float64) of how the uniform-geometry sample pass (csrc/smooth_ug.hip) settles a sample on a table row:
the first attempt -- SWEEPS projected sweeps that guess the active set, then up to PDAS primal-dual active-set iterations
(ug_pdas) -- and the up to PDAS_FLUSH further iterations a parked sample gets in the flush before the dual steps.

One iteration reads table entry `a`: the reduced set ap (rows of `a` in order, a dependent row dropped by the pivot rule)
and v = [multipliers on ap ; slacks off ap].  A row is bad when its multiplier is negative or its slack is below -tol.
  rule "release" (the device's): every bad row off ap joins; of the bad rows on ap exactly one leaves, the one with the
      most negative multiplier.  The device picks it as the largest unsigned key, key_i = the float32 bit pattern of v_i
      with the low three mantissa bits replaced by 7 - i: multipliers that agree in all but those bits tie, and the tie
      goes to the lowest row index.  The twin packs the same key from float32(v_i).
  rule "flip" (what it replaced, -DIRS_UG_FLIP_ALL=1): every bad row flips.
All samples of one state share W, so the 256 table entries are built once per state (as maps G_a: v = G_a r) and the
iterations run vectorised over the samples.
"""
import numpy as np

SWEEPS, PDAS, PDAS_FLUSH = 6, 3, 8          # csrc/smooth_ug.hip: IRS_UG_SWEEPS, IRS_UG_PDAS, IRS_UG_PDAS_FLUSH
OMEGA, PIVOT, TOL = 1.5, 1e-5, 1e-6         # the sweeps' relaxation, the table's pivot rule, the optimality tolerance (x max|r|)
PATH_FIRST, PATH_FLUSH, PATH_DUAL = 0, 1, 2  # settled in the first attempt / in the flush's iterations / left to the dual steps
HAND_IDX = np.array([1, 4, 2, 5])           # the commanded coordinates of the planar hand's state


def table_entry(W, a):
    """Entry `a` of the table as (on, G): the reduced set (rows of `a` in order; a row whose Schur complement on the rows
    accepted so far is below PIVOT W_ii drops out) and the map r -> v = [lam on the set ; slacks off it]."""
    nc = W.shape[0]
    S = []
    for j in range(nc):
        if not (a >> j) & 1:
            continue
        d = W[j, j] - (W[j, S].dot(np.linalg.solve(W[np.ix_(S, S)], W[S, j])) if S else 0.0)
        if d > PIVOT * W[j, j]:
            S.append(j)
    on = np.zeros(nc, bool)
    on[S] = True
    M = np.zeros((nc, nc))
    if S:
        M[np.ix_(S, S)] = -np.linalg.inv(W[np.ix_(S, S)])
    G = np.where(on[:, None], M, np.eye(nc) + W.dot(M))
    return on, G


def build_table(W):
    nc = W.shape[0]
    on = np.zeros((1 << nc, nc), bool)
    G = np.zeros((1 << nc, nc, nc))
    for a in range(1 << nc):
        on[a], G[a] = table_entry(W, a)
    return on, G


def bits(mask):
    """(B, nc) bool -> (B,) set as an integer, row i in bit i"""
    return (mask.astype(np.int64) << np.arange(mask.shape[-1])).sum(-1)


def sweep_guess(W, R, sweeps=SWEEPS):
    lam, g = np.zeros_like(R), R.copy()
    for _ in range(sweeps):
        for i in range(W.shape[0]):
            nw = np.maximum(lam[:, i] - g[:, i] * OMEGA / W[i, i], 0.0)
            g += W[:, i][None, :] * (nw - lam[:, i])[:, None]
            lam[:, i] = nw
    return bits(lam > 0)


def release_key(v, neg):
    """The device's key of every row: float32 bits of v_i, low three bits <- 7 - i, on the rows of `neg`; 0 elsewhere."""
    nc = v.shape[1]
    b = np.ascontiguousarray(v.astype(np.float32)).view(np.uint32)
    key = (b & np.uint32(0xFFFFFFF8)) | (np.uint32(7) - np.arange(nc, dtype=np.uint32))[None, :]
    return np.where(neg, key, np.uint32(0))


def iterate(table, R, a, cap, rule="release"):
    """Up to `cap` iterations from the sets `a` (B,) on the right-hand sides R (B, nc).  Returns (it, a, lam): the
    1-based iteration at which each sample settled (0: not within cap), the settled set or the set to try next, and the
    settled multipliers."""
    on_t, G_t = table
    B, nc = R.shape
    tol = TOL * np.maximum(np.abs(R).max(1), 1e-30)
    it = np.zeros(B, np.int64)
    a = a.copy()
    lam = np.zeros_like(R)
    for k in range(1, cap + 1):
        live = np.flatnonzero(it == 0)
        if len(live) == 0:
            break
        on = on_t[a[live]]
        v = np.einsum("bij,bj->bi", G_t[a[live]], R[live])
        bad = np.where(on, v, v + tol[live, None]) < 0
        ok = ~bad.any(1)
        lam[live[ok]] = np.where(on[ok], v[ok], 0.0)
        it[live[ok]] = k
        if rule == "flip":
            nxt = on ^ bad
        else:
            neg = bad & on
            worst = np.zeros_like(on)
            has = neg.any(1)
            worst[np.flatnonzero(has), 7 - (release_key(v, neg).max(1)[has] & 7).astype(np.int64)] = True
            nxt = (on & ~worst) | (bad & ~on)
        a[live] = bits(nxt)
    return it, a, lam


def classify(W, R, rule="release", sweeps=SWEEPS, pdas=PDAS, flush=PDAS_FLUSH, table=None):
    """Per sample: (it, path, lam).  it: the table row (1-based, counted through the flush's iterations) on which the
    sample settled, 0 for PATH_DUAL; lam: the settled multipliers (zeros for PATH_DUAL)."""
    table = build_table(W) if table is None else table
    it, a, lam = iterate(table, R, sweep_guess(W, R, sweeps), pdas, rule)
    path = np.where(it > 0, PATH_FIRST, PATH_DUAL)
    rest = np.flatnonzero(it == 0)
    if flush > 0 and len(rest):
        it2, _, lam2 = iterate(table, R[rest], a[rest], flush, rule)
        got = it2 > 0
        it[rest[got]] = pdas + it2[got]
        path[rest[got]] = PATH_FLUSH
        lam[rest[got]] = lam2[got]
    return it, path, lam


def dual_problems(sys_o, x, u, du):
    """W (nc, nc) of one state and the right-hand sides r (B, nc) of the commands u + du[s] (float64)."""
    B = du.shape[0]
    Dinv, b, J, phi = sys_o._qp(np.repeat(x[None], B, 0), u[None] + du)
    JD = J * Dinv
    W = JD[0].dot(J[0].T)
    assert np.allclose(np.einsum("bik,bjk->bij", JD, J), W[None], rtol=0, atol=1e-12 * np.abs(W).max()), "geometry moved with u"
    return W, phi - np.einsum("bik,bk->bi", JD, b)


def bench_rollout(orc):
    """The benchmark's T = 50 rollout: the planar hand at rest under its initial command."""
    HAND = orc.PlanarHandOracle
    sys_o = HAND(0.1)
    x0 = HAND.pack([0.0, 0.35, 0.0], [-np.pi / 4, -np.pi / 4], [np.pi / 4, np.pi / 4])
    u_trj = np.tile(x0[HAND_IDX], (50, 1))
    return sys_o, orc.rollout(sys_o, x0, u_trj), u_trj


def random_states(HAND, rng, k):
    """(X, U): separated, touching and deeply penetrating states with a command near the joint angles (the generator of
    the random-state tests of the sample pass)."""
    obj = np.stack([rng.uniform(-0.3, 0.3, k), rng.uniform(0.1, 0.7, k), rng.uniform(-1, 1, k)], 1)
    left = np.stack([rng.uniform(-2.2, -0.2, k), rng.uniform(-1.5, 0.5, k)], 1)
    right = np.stack([rng.uniform(0.2, 2.2, k), rng.uniform(-0.5, 1.5, k)], 1)
    X = np.zeros((k, 7))
    X[:, HAND.PERM] = np.hstack([obj, left, right])
    return X, X[:, HAND_IDX] + rng.normal(0, 0.1, (k, 4))
