"""The problems on which the tail-plan bound test (csrc/iterate.hip: plan_check_kernel, plan_check16_kernel<NN>) is
certified: every compiled state size, both kernels, and bounds that exactly one tail, one step or one ulp violates.
Plain NumPy, no torch.

The statement (tv_lqr.py:112-123 and the comment above plan_check_kernel).  Tail t is the QP that starts at step t
from the realised state x_new[t]; its unconstrained plan is the policy (K_s, k_s), s >= t, rolled out on the linear
model:  u_s = K_s x_s + k_s,  x_{s+1} = A_s x_s + B_s u_s + c_s,  x_t = x_new[t].  The QP bounds u_t .. u_{T-1} and
x_{t+1} .. x_T (x_t is data).  `plans` returns all of these values in np.longdouble, `within` says whether none of
them lies STRICTLY beyond its bound: a value equal to its bound is inside, and +-inf never binds.  The kernel's flag
is 0 where `within` is true and 1 otherwise.

Two data families, each a deterministic function of (n, m, T, seed):

  exact    small integers throughout.  Per step a signed permutation P_s, and B_s, K_s with entries in {-1, 0, 1}
           (control j idles -- column j of B_s is zero -- at the steps with (s + j) % 3 == 0); A_s = P_s - B_s K_s, so
           that A_s + B_s K_s = P_s; c_s, k_s in [-3, 3].  x_new is the consistent trajectory x_{t+1} = P_t x_t +
           B_t k_t + c_t from an integer x_0: all tails coincide and magnitudes grow at most linearly in T.  Every
           product and sum of either kernel, in any order and under any contraction, is exact in f64: the flag is a
           theorem, not a tolerance.
  generic  standard normal A_s, B_s, K_s, c_s, k_s, (A_s, B_s) scaled per step so that |A_s + B_s K_s|_2 <= 0.9;
           x_new standard normal per row, so every tail is different.  The family on which rounding differs between
           the kernels; a bound keeps MARGIN x (the component's range) from every value (the CPU test holds the f64
           evaluation, in both forms, to 1e-3 of that).

Bound shapes, all built from the statement's own values.  The rule: a finite bound sits at the extreme of all plan
entries of its component that are not meant to violate -- the entries of the case's plan outside the target set,
and the entries of the unmodified plan.

  touch     exact: every bound of all four vectors exactly at the extreme of its component: flag 0.  Then one bound
            at a time one np.nextafter inward: flag 1.  (kind, side, component) over x / u, lo / hi, first / last.
  snug      generic: the same with MARGIN in place of one ulp: every bound MARGIN x range outside the extreme (flag 0),
            then one bound MARGIN x range inside it (flag 1).
  one-tail  x_new[t*] alone is moved (an integer in the exact family); all bounds infinite but one (kind,
            component, side), at the extreme over every other tail (generic: MARGIN x range short of the moved
            tail's extreme): exactly tail t* violates.  t* from required_tails.
  one-step  k[s*] or c[s*] alone is spiked; the bound by the same rule; the only violating entries are at step s*,
            in the tails t <= s*.  s* = 0; s* = T-1 through k (the last control); s* = T-1 through c (X[T] alone).
            The first control of the last tail alone is the one-tail case t* = T-1 on a u bound.
  open      all four vectors +-inf but one slack finite entry; and +-inf mixed with finite slack values.  Flag 0.

A case is admitted (admit) only if the statement says that its target set is strictly beyond the bound and
everything else inside (exact: touching included; generic: by MARGIN x range on either side).  build raises
where a required case of a problem is not admitted; SEED records, per problem, the first seed at which all are.
"""
import functools

import numpy as np

LD = np.longdouble
MARGIN = 1e-6
LDS_BUDGET = 150 * 1024

# ------------------------------------------------------------------------------------------------ the statement


def plans(At, Bt, ct, K, k, x_new, tails=None):
    """(U, X) in np.longdouble: U[r, s, :] and X[r, s + 1, :] of tail t = tails[r] (default: every tail, r = t) for
    s >= t; NaN elsewhere (x_t itself is data, no plan entry)."""
    T, n, m = Bt.shape
    A, B, c, K, k, x_new = (np.asarray(a, dtype=LD) for a in (At, Bt, ct, K, k, x_new))
    ts = np.arange(T) if tails is None else np.asarray(tails, dtype=int)
    U = np.full((len(ts), T, m), np.nan, dtype=LD)
    X = np.full((len(ts), T + 1, n), np.nan, dtype=LD)
    x = np.zeros((len(ts), n), dtype=LD)
    for s in range(T):
        x[ts == s] = x_new[s]                       # tail s starts here, from the realised state
        on = ts <= s                                # one row per tail under way
        u = x[on] @ K[s].T + k[s]
        x[on] = x[on] @ A[s].T + u @ B[s].T + c[s]
        U[on, s], X[on, s + 1] = u, x[on]
    return U, X


def entries(plan):
    """(ok, Uv, Xv): the (rows, T) mask of the pairs (tail, step) that have plan entries, and the entries themselves,
    one row per pair: Uv[p] = U[t, s], Xv[p] = X[t, s + 1]."""
    U, X = plan
    ok = ~np.isnan(U[:, :, 0])
    return ok, U[ok], X[:, 1:][ok]


def within(plan, xlo, xhi, ulo, uhi):
    """True iff no plan entry lies strictly beyond its bound."""
    _, Uv, Xv = entries(plan)
    return not ((Uv < ulo).any() or (Uv > uhi).any() or (Xv < xlo).any() or (Xv > xhi).any())


# ------------------------------------------------------------------------------------------------ placement
def placement(n, m, T):
    """Which kernel plan_check_launch runs, restated: the fast one ("fast") if and only if n <= 16, m <= 16 and the
    closed loops fit LDS, T (n^2 + n + n m + m) 8 <= 150 KiB; else the serial one, "serial-n" (state size),
    "serial-lds" (LDS overflow, T <= 256: one pass) or "serial-multipass" (T > 256 = its block size)."""
    if n <= 16 and m <= 16 and T * (n * n + n + n * m + m) * 8 <= LDS_BUDGET:
        return "fast"
    if T > 256:
        return "serial-multipass"
    return "serial-n" if n > 16 or m > 16 else "serial-lds"


def pass_size(n, m, T):
    """Tails in flight per pass: fast kernel 4 per wave, as many waves as groups of four tails, at most 16; serial
    kernel one per thread, T rounded up to whole waves, at most 256."""
    if placement(n, m, T) == "fast":
        return 4 * min((T + 3) // 4, 16)
    return min((T + 63) // 64 * 64, 256)


def required_tails(n, m, T):
    """The t* of the one-tail cases present at this T: 0, 1, 3, 4 (a wave's four tails and the next wave's first), 63,
    64, 65, T-2, T-1, the first and last tail of the last pass, the tails either side of every pass boundary, and (T
    not a multiple of 4) the earliest tail of the last wave, whose later groups are dead."""
    G = pass_size(n, m, T)
    last = (T - 1) // G * G
    want = [0, 1, 3, 4, 63, 64, 65, T - 2, T - 1, last, last - 1, G - 1, G, (T - 1) // 4 * 4]
    return sorted({t for t in want if 0 <= t < T})


# ------------------------------------------------------------------------------------------------ shapes
FAST_SIZES = [(1, 2), (2, 1), (3, 16), (4, 4), (5, 2), (6, 1), (7, 4), (8, 8), (9, 2), (10, 16), (11, 1), (12, 4),
              (13, 13), (14, 2), (15, 4), (16, 16)]
T_MAIN = 37
EDGE_T = (1, 2, 3, 4, 5, 64, 65, 130, 200)
# (n, m, T) -> the side of the placement rule the shape is meant to reach.  n = m = 16 fits LDS up to T = 35.
SHAPES = {(n, m, 35 if (n, m) == (16, 16) else T_MAIN): "fast" for n, m in FAST_SIZES}
SHAPES.update({(n, m, T): "fast" for n, m in ((2, 1), (3, 2)) for T in EDGE_T})
SHAPES.update({(17, 3, 20): "serial-n", (32, 16, 9): "serial-n", (12, 4, 100): "serial-lds",
               (12, 4, 300): "serial-multipass", (20, 2, 300): "serial-multipass"})
FAMILIES = ("exact", "generic")
# (n, m, T, family) -> seed where it is not 0: the first at which every required case of the problem is admitted
# (find_seed; tests/test_plan_check_cpu.py admits every case at the recorded seed)
SEED = {(2, 1, 1, "exact"): 1, (2, 1, 2, "exact"): 1, (2, 1, 3, "exact"): 1, (2, 1, 130, "exact"): 1}


# ------------------------------------------------------------------------------------------------ problem data
@functools.lru_cache(maxsize=None)
def problem(n, m, T, family, seed=None):
    """dict(At, Bt, ct, K, k, x_new) in f64; x_new has T + 1 rows (row T is never a tail's start)."""
    seed = SEED.get((n, m, T, family), 0) if seed is None else seed
    rng = np.random.default_rng([n, m, T, FAMILIES.index(family), seed])
    if family == "exact":
        p = min(0.5, 2.0 / n)
        tri = lambda shape: rng.choice([-1.0, 0.0, 1.0], p=[p / 2, 1 - p, p / 2], size=shape)
        P = np.zeros((T, n, n))
        for s in range(T):
            P[s, np.arange(n), rng.permutation(n)] = rng.choice([-1.0, 1.0], size=n)
        B, K = tri((T, n, m)), tri((T, m, n))
        for s in range(T):
            B[s][:, [j for j in range(m) if (s + j) % 3 == 0]] = 0.0
        A = P - B @ K
        c, k = rng.integers(-3, 4, size=(T, n)).astype(float), rng.integers(-3, 4, size=(T, m)).astype(float)
        x = np.zeros((T + 1, n))
        x[0] = rng.integers(-3, 4, size=n)
        for t in range(T):
            x[t + 1] = P[t] @ x[t] + B[t] @ k[t] + c[t]
    else:
        A, B, K = rng.normal(size=(T, n, n)), rng.normal(size=(T, n, m)), rng.normal(size=(T, m, n))
        for s in range(T):
            f = 0.9 / max(np.linalg.norm(A[s] + B[s] @ K[s], 2), 0.9)
            A[s] *= f
            B[s] *= f
        c, k, x = rng.normal(size=(T, n)), rng.normal(size=(T, m)), rng.normal(size=(T + 1, n))
    out = dict(At=A, Bt=B, ct=c, K=K, k=k, x_new=x)
    for v in out.values():
        v.setflags(write=False)
    return out


DATA_KEYS = ("At", "Bt", "ct", "K", "k", "x_new")


def case_data(c):
    """The six arrays of a case: its problem's, with the case's own x_new / k / ct in place."""
    d = dict(problem(c["n"], c["m"], c["T"], c["family"], c["seed"]))
    d.update(c["override"])
    return d


@functools.lru_cache(maxsize=8)
def _base_plan(n, m, T, family, seed):
    d = problem(n, m, T, family, seed)
    return plans(*[d[k] for k in DATA_KEYS])


def case_plan(c):
    """The statement's plan of a case.  Tail t sees only x_new[t]: where the case moves x_new[t*] alone, only that
    tail is evaluated anew."""
    U, X = _base_plan(c["n"], c["m"], c["T"], c["family"], c["seed"])
    if not c["override"]:
        return U, X
    d = case_data(c)
    if set(c["override"]) == {"x_new"}:
        t = c["target"]["t"]
        U, X = U.copy(), X.copy()
        U[t:t + 1], X[t:t + 1] = plans(*[d[k] for k in DATA_KEYS], tails=[t])
        return U, X
    return plans(*[d[k] for k in DATA_KEYS])


# ------------------------------------------------------------------------------------------------ admission
def _values(plan, kind):
    """(T, T, width): entry [t, s] = U[t, s] or X[t, s + 1]."""
    return plan[0] if kind == "u" else plan[1][:, 1:]


def _nanptp(v):
    return float(np.nanmax(v) - np.nanmin(v))


def verdict(c, plan=None):
    """(beyond, unclear) of the case's bounds on the statement's plan: per finite bound (kind, side, component) the
    boolean (T, T) mask of the entries strictly beyond it, and the number of entries that are neither beyond nor
    inside by the case's margin (exact family: margin 0, touching is inside).  An infinite bound has no entry."""
    plan = case_plan(c) if plan is None else plan
    xlo, xhi, ulo, uhi = c["bounds"]
    generic = c["family"] == "generic"
    beyond, unclear = {}, 0
    ok = ~np.isnan(plan[0][:, :, 0])
    for kind, lo, hi in (("x", xlo, xhi), ("u", ulo, uhi)):
        v = _values(plan, kind)
        for side, b in (("lo", lo), ("hi", hi)):
            for i in np.flatnonzero(np.isfinite(b)):
                vi = v[:, :, i][ok]
                d = vi - b[i] if side == "lo" else b[i] - vi              # signed distance inside
                mg = c["margin"][kind][i]
                far = np.zeros(ok.shape, dtype=bool)
                far[ok] = d < -mg if generic else d < 0
                beyond[kind, side, int(i)] = far
                unclear += int(((d < mg) & (d >= -mg)).sum()) if generic else 0
    return beyond, unclear


def admit(c, plan=None):
    """None if the case is admitted, else the reason.  Admitted: no entry within the margin of a bound; the entries
    beyond a bound are exactly none (want 0), or lie all in the target set, on the target's (kind, component, side)
    alone, and are at least one (want 1); for a one-step case every target entry is beyond."""
    beyond, unclear = verdict(c, plan)
    if unclear:
        return "%d entries within the margin of a bound" % unclear
    n_beyond = sum(int(b.sum()) for b in beyond.values())
    if c["want"] == 0:
        return None if n_beyond == 0 else "%d entries beyond a bound, none wanted" % n_beyond
    tg = c["target"]
    hit = beyond[tg["kind"], tg["side"], tg["comp"]]
    if int(hit.sum()) != n_beyond:
        return "entries beyond a bound off the target's (kind, component, side)"
    if not hit.any():
        return "nothing beyond the bound"
    mask = target_mask(c)
    if (hit & ~mask).any():
        return "entries beyond the bound outside the target set"
    if c["shape"] == "one-step" and not hit[mask].all():
        return "a target entry inside the bound"
    return None


def target_mask(c):
    """(T, T) boolean [t, s]: the entries of the target's (kind, component) that may lie beyond the bound."""
    T, tg = c["T"], c["target"]
    mask = np.zeros((T, T), dtype=bool)
    if tg["t"] is not None:
        mask[tg["t"], tg["t"]:] = True                       # one tail: any of its entries
    elif tg["s"] is not None:
        mask[:tg["s"] + 1, tg["s"]] = True                   # one step: that step, in the tails that reach it
    else:
        mask[np.triu_indices(T)] = True                      # touch / snug: wherever the extreme is attained
    return mask


class NotAdmitted(Exception):
    pass


# ------------------------------------------------------------------------------------------------ the cases
def _inf_bounds(n, m):
    return [np.full(n, -np.inf), np.full(n, np.inf), np.full(m, -np.inf), np.full(m, np.inf)]


_SLOT = {("x", "lo"): 0, ("x", "hi"): 1, ("u", "lo"): 2, ("u", "hi"): 3}


def _extreme(v, side):
    return np.nanmin(v) if side == "lo" else np.nanmax(v)


def _f64_outward(e, side):
    """The f64 nearest to the longdouble e on the side away from the interior (exact family: e itself)."""
    b = float(e)
    if side == "hi" and b < e:
        b = np.nextafter(b, np.inf)
    if side == "lo" and b > e:
        b = np.nextafter(b, -np.inf)
    return b


def build(n, m, T, family, seed=None):
    """Every case of one problem, each admitted; NotAdmitted where a required one is not."""
    seed = SEED.get((n, m, T, family), 0) if seed is None else seed
    d = problem(n, m, T, family, seed)
    base = _base_plan(n, m, T, family, seed)
    exact = family == "exact"
    sgn = {"lo": -1.0, "hi": 1.0}
    rng_of = {kind: np.array([_nanptp(_values(base, kind)[:, :, i]) for i in range(w)])
              for kind, w in (("x", n), ("u", m))}
    # the margin of a component: MARGIN x its range (a constant component: x its size, at least 1)
    margin = {kind: (np.zeros_like(r) if exact else MARGIN * np.where(r > 0, r, 1.0)) for kind, r in rng_of.items()}
    base_ext = {(kind, side): np.array([_extreme(_values(base, kind)[:, :, i], side) for i in range(w)])
                for kind, w in (("x", n), ("u", m)) for side in ("lo", "hi")}
    cases = []

    def new(shape, want, bounds, target, override=None):
        c = dict(id="%s-%d-%d-%d-%s-%02d" % (family, n, m, T, shape, len(cases)), n=n, m=m, T=T, family=family,
                 seed=seed, shape=shape, want=want, bounds=[np.array(b, dtype=float) for b in bounds], target=target,
                 override=override or {}, margin=margin, placement=placement(n, m, T))
        return c

    def tgt(t=None, s=None, kind=None, comp=None, side=None, via=None):
        return dict(t=t, s=s, kind=kind, comp=comp, side=side, via=via)

    def add(c, plan=None, required=True):
        why = admit(c, plan)
        if why is None:
            cases.append(c)
        elif required:
            raise NotAdmitted("%s %s: %s" % (c["id"], c["target"], why))
        return why is None

    # ---- touch / snug: every bound at its component's extreme (generic: one margin outside)
    full = _inf_bounds(n, m)
    for (kind, side), slot in _SLOT.items():
        v = _values(base, kind)
        for i in range(len(full[slot])):
            e = _extreme(v[:, :, i], side)
            full[slot][i] = _f64_outward(e, side) if exact else float(e) + sgn[side] * 2.0 * margin[kind][i]
    name = "touch" if exact else "snug"
    add(new(name, 0, full, tgt()), base)
    combos = []
    for kind, w in (("x", n), ("u", m)):
        for side in ("lo", "hi"):
            for i in sorted({0, w - 1}):
                combos.append((kind, i, side))
    for kind, i, side in combos:
        b = [a.copy() for a in full]
        slot = _SLOT[kind, side]
        e = _extreme(_values(base, kind)[:, :, i], side)
        b[slot][i] = np.nextafter(b[slot][i], -sgn[side] * np.inf) if exact else float(e) - sgn[side] * 2.0 * margin[kind][i]
        # (generic: a second entry within the margins of the moved bound is possible; the full case above is the
        # required one, and the CPU test holds the family to one admitted inward case per kind and side)
        add(new(name + "-in", 1, b, tgt(kind=kind, comp=i, side=side)), base, required=exact)

    # ---- one bound placed by the rule on a modified plan
    def one_bound(shape, target, override, plan, strict_all):
        """The case with the single bound of `target` placed by the rule, or None where the target is not beyond."""
        kind, i, side = target["kind"], target["comp"], target["side"]
        c = new(shape, 1, _inf_bounds(n, m), target, override)
        mask = target_mask(c)
        v = _values(plan, kind)[:, :, i]
        others = np.concatenate([v[~mask & ~np.isnan(v)], _values(base, kind)[:, :, i][np.triu_indices(T)]])
        e = _extreme(others, side)
        tv = v[mask]
        # the target entry the bound has to be short of: the nearest (every target entry violates) or the furthest
        far = _extreme(tv, side)
        near = _extreme(tv, "hi" if side == "lo" else "lo")
        t_ref = near if strict_all else far
        if exact:
            b = float(e)
        else:
            b = float(t_ref) - sgn[side] * 2.0 * margin[kind][i]
        c["bounds"][_SLOT[kind, side]][i] = b
        return c

    def search(shape, t=None, s=None, via=None, pref=0, kinds=("x", "u")):
        """Try (kind, component, side), starting from the pref-th, and the component and sign of the move, until a
        case is admitted."""
        trips = [(kind, i, side) for kind in kinds for i in sorted({0, (n if kind == "x" else m) - 1,
                                                                    (n if kind == "x" else m) // 2})
                 for side in ("lo", "hi")]
        trips = trips[pref % len(trips):] + trips[:pref % len(trips)]
        rows = {}
        for kind, i, side in trips:
            scale = max(float(np.max(rng_of["x"])), float(np.max(rng_of["u"])), 1.0)
            delta0 = float(2 * np.ceil(scale) + 1) if exact else 20.0 * scale
            if via == "x_new":
                moves = [(j, sg) for j in range(n) for sg in (1.0, -1.0)]
            else:                                   # the spike goes straight into the bounded component
                moves = [(i, sgn[side])]
            for j, sg in moves:
                arr = np.array(d[via])
                row = t if via == "x_new" else s
                arr[row, j] += sg * delta0
                c0 = dict(n=n, m=m, T=T, family=family, seed=seed, override={via: arr},
                          target=tgt(t=t, s=s, kind=kind, comp=i, side=side, via=via))
                if via == "x_new":
                    # the moved tail alone, first: is its extreme beyond everything the unmodified plan holds?
                    if (j, sg) not in rows:
                        rows[j, sg] = plans(*[c0["override"].get(key, d[key]) for key in DATA_KEYS], tails=[t])
                    far = _extreme(_values(rows[j, sg], kind)[0, :, i], side)
                    if not sgn[side] * (far - base_ext[kind, side][i]) > 3.0 * margin[kind][i]:
                        continue
                plan = case_plan(c0)
                c = one_bound(shape, c0["target"], c0["override"], plan, strict_all=s is not None)
                if add(c, plan, required=False):
                    return True
        raise NotAdmitted("%s-%d-%d-%d %s t*=%s s*=%s via %s: no admitted case" % (family, n, m, T, shape, t, s, via))

    for q, t in enumerate(required_tails(n, m, T)):
        search("one-tail", t=t, via="x_new", pref=q)
    # the first control of the last tail alone: tail T-1 has one control, and the bound is on u
    search("one-tail", t=T - 1, via="x_new", pref=T, kinds=("u",))
    # one step: s* = 0 (exact: through k, where the control idles at step 0 and nothing propagates; generic: through
    # c, where the closed loop contracts what propagates), the last control, the terminal state
    search("one-step", s=0, via="k" if exact else "ct", pref=1, kinds=("u",) if exact else ("x",))
    search("one-step", s=T - 1, via="k", pref=2, kinds=("u",))
    search("one-step", s=T - 1, via="ct", pref=3, kinds=("x",))

    # ---- open
    slack = lambda kind, i, side: float(_extreme(_values(base, kind)[:, :, i], side)) + sgn[side] * 10.0 * (
        1.0 + rng_of[kind][i])
    b = _inf_bounds(n, m)
    b[1][n - 1] = slack("x", n - 1, "hi")
    add(new("open", 0, b, tgt()), base)
    b = _inf_bounds(n, m)
    for (kind, side), slot in _SLOT.items():
        for i in range(len(b[slot])):
            if (i + slot) % 2 == 0:
                b[slot][i] = slack(kind, i, side)
    add(new("open-mixed", 0, b, tgt()), base)
    return cases


@functools.lru_cache(maxsize=None)
def cases(n, m, T, family):
    return build(n, m, T, family)


def find_seed(n, m, T, family, limit=50):
    for seed in range(limit):
        try:
            build(n, m, T, family, seed)
            return seed
        except NotAdmitted:
            pass
    raise NotAdmitted("no seed below %d admits every case of %s" % (limit, (n, m, T, family)))


def describe(c):
    """One line for a failure message: id, family, target and the placement the case is meant to reach."""
    tg = c["target"]
    return "%s [%s, %s, want %d] target t*=%s s*=%s %s[%s] %s via %s; placement %s" % (
        c["id"], c["family"], c["shape"], c["want"], tg["t"], tg["s"], tg["kind"], tg["comp"], tg["side"], tg["via"],
        c["placement"])
