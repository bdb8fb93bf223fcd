"""Which lane reads which sample: a restatement of the sample loops of csrc/smooth.hip and csrc/smooth_ug.hip, the
exactly summable samples that make a lost, doubled or mis-rowed sample visible, and the shapes that reach every
launch geometry.  NumPy only (with the f64 oracle of oracle/irs_oracle.py for the steps); the geometry itself comes from the library's own planner (irs_smooth_geometry) and is
passed in as a dict -- nothing here restates the planner.

A launch is a grid (nblk, T).  Within a timestep every loop hands 64 CONSECUTIVE samples to one wave at a time (lane l
of the wave reads sample start + l), so ownership is stated per wave slot:

    owners(geom, N, rng) -> dict of equally long int arrays
        wg, wave, trip, sub   who: workgroup, wave in it, trip of that wave's loop, sample slot within the trip
        start, stop           samples [start, stop) are read by lanes 0 .. stop - start - 1; stop <= start: a tail slot,
                              whose lanes load the clamped row s_end - 1 and must contribute nothing

The five loops (line numbers: the kernels as of this file's commit):
  * lanes, light, samples supplied (smooth.hip:365-398, U = 4): lane tid of workgroup b starts at s_begin + tid and
    strides by 4 BLOCK; slot uu of a trip is sample s0 + uu BLOCK, valid while < s_end, else clamped and zeroed;
  * lanes, one sample per trip (smooth.hip:365, U = 1: heavy kernels, and light ones with device-drawn samples):
    s_begin + tid + k BLOCK, the next row prefetched (smooth.hip:350-363);
  * matrix-core Gram (smooth.hip:95-97): wave w takes s_begin + 64 w + k BLOCK, lane l its sample l;
  * contact, wave-dealt (smooth.hip:338-346 next_s0; smooth.hip:210-213 block_of with the parked-sample ring): trip k
    of wave w takes 64-sample block 4 k + w of the workgroup; in workgroup 0 the last wave sits out after wg0_rr
    trips and the other three take blocks 4 rr + 3 (k - rr) + w;
  * uniform geometry (smooth_ug.hip:624-628): the V = 8 nblk waves of a timestep are numbered `me` -- workgroup 0's
    waves 0..6, then 8 b - 1 + w, the nominal wave (workgroup 0, wave 7) last -- and block_of(k) deals rounds 0, 1 to
    all but the nominal wave and every later round to all V.
Workgroup b of the first four families owns [s_begin, s_end) = chunk0 + [(b-1) chunk, b chunk) cut at N (smooth.hip:78-79).
"""
import numpy as np

from oracle import irs_oracle as orc

LIGHT, HEAVY, GRAM, WAVE_DEALT, PARKED, UG = ("lanes_light", "lanes_heavy", "gram_matrix_core", "contact_wave_dealt",
                                             "contact_parked", "uniform_geometry")
NEVER = 0x7fffffff
UG_NOM_ROUNDS = 2          # smooth_ug.hip: kUgNomRounds
ZERO_ORDER_AB, FIRST_ORDER, ZERO_ORDER_B = 0, 1, 2

# include/irs_hip.h: irs_model_id, with (n, m) and whether the step is a contact QP
MODELS = {
    "pendulum": (0, 2, 1, False), "pendulum_h04": (0, 2, 1, False), "quadrotor": (1, 12, 4, False), "bicycle": (2, 5, 2, False),
    "three_cart": (3, 6, 2, False), "planar_hand_pgs": (4, 7, 4, True), "box_pivot_pgs": (5, 5, 2, True),
    "box_on_box": (6, 4, 2, True), "box_push_pgs": (7, 5, 2, True), "planar_hand": (8, 7, 4, True),
    "box_pivot": (9, 5, 2, True), "box_push": (10, 5, 2, True),
}


def wg_ranges(geom, N):
    """[s_begin, s_end) of every workgroup of a timestep (smooth.hip:78-79); the uniform-geometry family has none."""
    b = np.arange(geom["nblk"])
    beg = np.where(b == 0, 0, geom["chunk0"] + (b - 1) * geom["chunk"])
    end = np.minimum(N, np.where(b == 0, geom["chunk0"], geom["chunk0"] + b * geom["chunk"]))
    return beg, end


def _table(keep, prefix=None, **cols):
    """The visited slots of the (workgroup, wave, trip[, slot]) grids; a wave's trips must be a prefix of its grid."""
    first = prefix if prefix is not None else keep[..., 0] if keep.ndim == 4 else keep
    assert not first[:, :, -1].any() and (first[:, :, 1:] <= first[:, :, :-1]).all()
    return {k: np.broadcast_to(v, keep.shape)[keep] for k, v in cols.items()}


def owners(geom, N, rng=False):
    fam, block, nblk = geom["family"], geom["block"], geom["nblk"]
    if fam == UG:
        V, nblocks = nblk * 8, (N + 63) // 64
        b, w = np.arange(nblk)[:, None, None], np.arange(8)[None, :, None]
        k = np.arange(nblocks // max(V - 1, 1) + UG_NOM_ROUNDS + 2)[None, None, :]
        nominal = (b == 0) & (w == 7)
        me = np.where(nominal, V - 1, np.where(b == 0, w, b * 8 - 1 + w))
        blk = np.where(k < UG_NOM_ROUNDS, k * (V - 1) + me, UG_NOM_ROUNDS * (V - 1) + (k - UG_NOM_ROUNDS) * V + me)
        blk = np.where(nominal & (k < UG_NOM_ROUNDS), blk[:, :, UG_NOM_ROUNDS:UG_NOM_ROUNDS + 1], blk)
        # (the nominal wave starts at round kUgNomRounds: its first two grid entries repeat that block and are dropped)
        keep = (blk < nblocks) & ~(nominal & (k < UG_NOM_ROUNDS))      # `fresh` (smooth_ug.hip:649)
        return _table(keep, prefix=blk < nblocks, wg=b, wave=w, trip=k, sub=0 * k, start=blk * 64, stop=np.minimum(blk * 64 + 64, N))
    NW = block // 64
    U = 4 if (fam == LIGHT and not rng) else 1
    dealt = fam in (WAVE_DEALT, PARKED)
    beg, end = wg_ranges(geom, N)
    b, w = np.arange(nblk)[:, None, None], np.arange(NW)[None, :, None]
    k = np.arange(max(int((end - beg).max()), 0) // 64 + 2)[None, None, :]     # more trips than any wave makes
    s_begin, s_end = beg[:, None, None], end[:, None, None]
    if dealt:
        rr = np.where(b == 0, geom["wg0_rr"], NEVER)
        blk = np.where(k < rr, NW * k + w, NW * rr + (NW - 1) * (k - rr) + w)
        start = np.where((w == NW - 1) & (k >= rr), s_end, s_begin + 64 * blk)     # the nominal wave sits out
    else:
        start = s_begin + 64 * w + k * (block * U)
    keep = start < s_end                                               # the loop condition of the wave's first lane
    uu = np.arange(U)[None, None, None, :]
    s0 = start[..., None] + uu * block
    keep4 = np.broadcast_to(keep[..., None], s0.shape)
    return _table(keep4, wg=b[..., None], wave=w[..., None], trip=k[..., None], sub=uu, start=s0,
                  stop=np.minimum(s0 + 64, s_end[..., None]))


def reader_count(own, N):
    """How many lanes read each of the N samples (must be 1 everywhere)."""
    live = own["stop"] > own["start"]
    diff = np.zeros(N + 1, int)
    np.add.at(diff, own["start"][live], 1)
    np.add.at(diff, own["stop"][live], -1)
    return np.cumsum(diff[:N])


def tiles(own, N):
    """True iff the live slots partition [0, N): the cheap form of reader_count(own, N) == 1."""
    live = own["stop"] > own["start"]
    st, sp = own["start"][live], own["stop"][live]
    o = np.argsort(st, kind="stable")
    st, sp = st[o], sp[o]
    return st.size > 0 and st[0] == 0 and sp[-1] == N and bool((st[1:] == sp[:-1]).all())


def trips_per_lane(geom, N, rng=False):
    """The most samples any one lane adds up."""
    own = owners(geom, N, rng)
    live = own["stop"] > own["start"]
    return int(np.bincount(own["wg"][live] * 16 + own["wave"][live]).max())


def boundary_samples(geom, N, own):
    """First and last sample of every workgroup range, of every wave slot (a wave's 64-sample block of one trip)."""
    live = own["stop"] > own["start"]
    s = [own["start"][live], own["stop"][live] - 1]
    if geom["family"] != UG:
        beg, end = wg_ranges(geom, N)
        ok = end > beg
        s += [beg[ok], end[ok] - 1]
    return np.unique(np.concatenate(s))


def clamp_row(geom, N, own, s):
    """The row a lane past the end of sample s's range would load: s_end - 1 of its workgroup (N - 1: uniform geometry)."""
    if geom["family"] == UG:
        return N - 1
    beg, end = wg_ranges(geom, N)
    b = int(np.searchsorted(end, s, side="right"))
    return int(end[b]) - 1


# ------------------------------------------------------------------------------------------------ exact samples
def dyadic_samples(T, N, width, seed):
    """(T, N, width) integers k in [-4, 4] -- the samples are k 2^-5 -- every timestep another draw, no all-zero row."""
    g = seed if isinstance(seed, np.random.Generator) else np.random.default_rng(seed)
    k = g.integers(-4, 5, size=(T, N, width))
    while True:
        dead = ~k.any(axis=2)
        if not dead.any():
            return k
        k[dead] = g.integers(-4, 5, size=(int(dead.sum()), width))


def as_f32(k):
    return (k * 2.0 ** -5).astype(np.float32)


def exact_blocks(k):
    """(upper Gram (T, w(w+1)/2), sum (T, w)) of the samples k 2^-5, by integer arithmetic: exact, and exactly what an
    f32 accumulation in ANY order gives while 16 N < 2^24."""
    assert 16 * k.shape[1] < 2 ** 24
    k = k.astype(np.int64)
    iu = np.triu_indices(k.shape[2])
    G = np.einsum("tni,tnj->tij", k, k)[:, iu[0], iu[1]]
    return G * 2.0 ** -10, k.sum(axis=1) * 2.0 ** -5


def mutate(k, t, s, how, clamp):
    """The samples as a faulty loop would see them: sample s of timestep t dropped, read twice, or replaced by the
    clamped row.  Returned as (k', weights): weights multiply each sample's contribution."""
    k2, w = k.copy(), np.ones(k.shape[:2])
    if how == "drop":
        w[t, s] = 0
    elif how == "twice":
        w[t, s] = 2
    else:
        k2[t, s] = k[t, clamp]
    return k2, w


def sums_layout(n, m, mode, contact):
    """Slices of `sums` (include/irs_hip.h) for a zero-order mode: (perturbed columns of z=[dx|du], Gram, z df', sum z)."""
    z0 = n if mode == ZERO_ORDER_B else 0
    nz = n + m - z0
    ng = nz * (nz + 1) // 2
    return dict(z0=z0, nz=nz, gram=slice(0, ng), zdf=slice(ng, ng + nz * n),
                sumz=slice(ng + nz * n, ng + nz * n + nz) if contact else None)


# ------------------------------------------------------------------------------------------------ the cases
# (id, model, mode, T, N, sources, what the planner must answer).  `want` keys: family, branch, block, nblk, wg0_rr,
# chunk0, chunk as values; min_nblk, min_rr as lower bounds; empty: workgroups without a sample; last: samples of the
# last workgroup; min_rounds: trips of the busiest wave, nominal_slots: blocks the uniform-geometry kernel's nominal wave
# owns (both through `owners`).  sources: "s" supplied, "r" device-drawn.
def _rows():
    rows = []

    def add(tag, model, mode, T, Ns, src, **want):
        for N in (Ns if isinstance(Ns, (list, tuple)) else [Ns]):
            rows.append(dict(id="%s-%s-m%d-T%d-N%d" % (tag, model, mode, T, N), model=model, mode=mode, T=T, N=N,
                             sources=src, want=want))

    # (first-order: the pendulum with a step of 0.4 s -- its Jacobian varies with the sample through h cos(theta) only, and
    # at h = 0.05 one swapped sample in 16384 moves the sum by less than f32 resolves)
    for mode in (ZERO_ORDER_AB, FIRST_ORDER, ZERO_ORDER_B):
        add("light1024", "pendulum_h04" if mode == FIRST_ORDER else "pendulum", mode, 3, [1, 1023, 1024, 1025, 4095, 4096, 4097, 16384], "s",
            family=LIGHT, block=1024, nblk=1)
    add("light-many", "pendulum", ZERO_ORDER_AB, 1, 16385, "s", family=LIGHT, block=256, nblk=17, last=1)
    add("light-many", "pendulum_h04", FIRST_ORDER, 30, 20000, "s", family=LIGHT, block=256, min_nblk=2)
    add("light-many", "pendulum", ZERO_ORDER_AB, 30, 20000, "s", family=LIGHT, block=256, min_nblk=2)
    for mode in (ZERO_ORDER_AB, ZERO_ORDER_B):
        add("light-rng", "pendulum", mode, 1, 257, "r", family=LIGHT, block=256)
        add("light-rng", "pendulum", mode, 1, 1025, "r", family=LIGHT, block=256, min_nblk=2)
    add("light-rng", "pendulum", ZERO_ORDER_B, 30, 3000, "r", family=LIGHT, block=256)
    heavy_N = [1, 255, 256, 257, 1025]
    add("heavy", "bicycle", ZERO_ORDER_AB, 2, heavy_N, "sr", family=HEAVY, block=256)
    add("heavy", "bicycle", FIRST_ORDER, 2, heavy_N, "sr", family=HEAVY, block=256)
    add("heavy", "three_cart", FIRST_ORDER, 2, heavy_N, "sr", family=HEAVY, block=256)
    add("heavy", "quadrotor", FIRST_ORDER, 2, heavy_N, "sr", family=HEAVY, block=256)
    add("heavy-3wg", "quadrotor", FIRST_ORDER, 2, 2049, "sr", family=HEAVY, block=256, min_nblk=3)
    add("heavy-3wg", "bicycle", ZERO_ORDER_AB, 2, 2049, "sr", family=HEAVY, block=256, min_nblk=3)
    gram_N = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1025]
    add("gram", "quadrotor", ZERO_ORDER_AB, 2, gram_N, "sr", family=GRAM, block=256)
    add("gram", "three_cart", ZERO_ORDER_AB, 2, gram_N, "sr", family=GRAM, block=256)
    add("gram", "planar_hand", ZERO_ORDER_AB, 2, gram_N, "sr", family=GRAM, block=256)
    for model, fam, modes in (("box_pivot", WAVE_DEALT, (ZERO_ORDER_B, FIRST_ORDER)),
                              ("planar_hand_pgs", WAVE_DEALT, (ZERO_ORDER_B,)),
                              ("planar_hand", PARKED, (ZERO_ORDER_B, FIRST_ORDER))):
        # planar_hand runs this family under IRS_UG=0 (the test sets it per call)
        for mode in modes:
            add("single", model, mode, 1, 1, "sr", family=fam, branch="none", nblk=1)
            add("plain", model, mode, 1, 257, "sr", family=fam, branch="none", nblk=2, last=1)
            # wave trips (wg0_rr finite).  The planner deals the nominal step ONE trip, so the
            # "nominal cost" re-planning and its empty workgroups are out of reach of any (T, N): the sweep of
            # tests/test_smooth_geometry_cpu.py asserts that, and must be given cases the day it stops being true
            add("trips-min", model, mode, 1, 449, "sr", family=fam, branch="trips", chunk0=448, chunk=64, wg0_rr=1,
                nblk=2, last=1)
            add("trips", model, mode, 86, 513, "sr", family=fam, branch="trips", chunk0=448, chunk=128, wg0_rr=1)
            add("trips", model, mode, 26, 2305, "sr", family=fam, branch="trips", nblk=5, wg0_rr=1)
            add("trips", model, mode, 65, 897, "sr", family=fam, branch="trips", chunk0=448, chunk=512, wg0_rr=1)
            add("trips-rr2", model, mode, 43, 1473, "sr", family=fam, branch="trips", wg0_rr=2, nblk=3)
            add("trips-rr2", model, mode, 128, 1001, "sr", family=fam, branch="trips", wg0_rr=2)
    for mode in (ZERO_ORDER_B, FIRST_ORDER):
        add("ug", "planar_hand", mode, 1, [1, 63, 64, 65, 449, 513], "sr", family=UG, block=512)
        add("ug", "planar_hand", mode, 26, 2305, "sr", family=UG, block=512, min_nblk=2)
        add("ug", "planar_hand", mode, 64, 897, "sr", family=UG, block=512, min_nblk=2)
        add("ug-1wg", "planar_hand", mode, 200, 577, "sr", family=UG, block=512, nblk=1, min_rounds=2)
        # three rounds of the deal and the nominal wave (which sits out two, then joins) owning a block: one workgroup,
        # and two
        add("ug-1wg-joins", "planar_hand", mode, 200, 1409, "sr", family=UG, block=512, nblk=1, min_rounds=3,
            nominal_slots=1)
        add("ug-joins", "planar_hand", mode, 100, 2945, "sr", family=UG, block=512, nblk=2, min_rounds=3,
            nominal_slots=1)
    return rows


CASES = {r["id"]: r for r in _rows()}


def needs_general_kernel(case):
    """The planar hand's general (parked-sample / matrix-core) kernels run its u-only modes only under IRS_UG=0."""
    return case["model"] == "planar_hand" and case["want"]["family"] == PARKED


def admit(case, geom, N):
    """Why `geom` is not the geometry the case names (None: it is)."""
    w = case["want"]
    for key in ("family", "branch", "block", "nblk", "wg0_rr", "chunk0", "chunk"):
        if key in w and geom[key] != w[key]:
            return "%s: %s is %r, the case needs %r" % (case["id"], key, geom[key], w[key])
    if geom["nblk"] < w.get("min_nblk", 1):
        return "%s: nblk %d < %d" % (case["id"], geom["nblk"], w["min_nblk"])
    if "min_rr" in w and not (w["min_rr"] <= geom["wg0_rr"] < NEVER):
        return "%s: wg0_rr %d, the case needs a finite one >= %d" % (case["id"], geom["wg0_rr"], w["min_rr"])
    if geom["family"] != UG:
        beg, end = wg_ranges(geom, N)
        if "empty" in w and int((end <= beg).sum()) != w["empty"]:
            return "%s: %d empty workgroups, the case needs %d" % (case["id"], int((end <= beg).sum()), w["empty"])
        if "last" in w and int(end[-1] - beg[-1]) != w["last"]:
            return "%s: the last workgroup holds %d samples, not %d" % (case["id"], int(end[-1] - beg[-1]), w["last"])
    if "min_rounds" in w or "nominal_slots" in w:
        own = owners(geom, N)
        rounds = int(own["trip"].max()) + 1
        nominal = int(((own["wg"] == 0) & (own["wave"] == 7) & (own["stop"] > own["start"])).sum())
        if rounds < w.get("min_rounds", 0):
            return "%s: the deal has %d rounds, the case needs %d" % (case["id"], rounds, w["min_rounds"])
        if nominal < w.get("nominal_slots", 0):
            return "%s: the nominal wave owns %d blocks, the case needs %d" % (case["id"], nominal, w["nominal_slots"])
    return None


# ------------------------------------------------------------------------------------------------ the problems
# model -> (device class of irs_mpc_amd, its arguments, the oracle)
SYSTEMS = {
    "pendulum": ("PendulumDynamics", (0.05,), {}, lambda: orc.PendulumOracle(0.05)),
    "pendulum_h04": ("PendulumDynamics", (0.4,), {}, lambda: orc.PendulumOracle(0.4)),
    "quadrotor": ("QuadrotorDynamics", (0.05,), {}, lambda: orc.QuadrotorOracle(0.05)),
    "bicycle": ("BicycleDynamics", (0.1,), {}, lambda: orc.BicycleOracle(0.1)),
    "three_cart": ("ThreeCartDynamics", (0.05,), {}, lambda: orc.ThreeCartOracle(0.05)),
    "planar_hand": ("PlanarHandDynamics", (0.1,), {}, lambda: orc.PlanarHandOracle(0.1)),
    "planar_hand_pgs": ("PlanarHandDynamics", (0.1,), dict(contact_solver="pgs"),
                        lambda: orc.PlanarHandOracle(0.1, pgs_iters=50)),
    "box_pivot": ("BoxPivotingDynamics", (0.1,), {}, lambda: orc.BoxPivotOracle(0.1)),
}
_memo = {}


def oracle_system(model):
    if model not in _memo:
        _memo[model] = SYSTEMS[model][3]()
    return _memo[model]


def nominal(model, T, separated=False, first_order=False):
    """(x_trj (T + 1, n), u_trj (T, m)): one nominal point repeated -- the samples differ per timestep, the point need
    not.  Contact models: the settled grasp of the planar hand (loaded contacts: 8-40 % of the samples are parked) and
    the hand at the box's side; separated=True: a pose where no command in range makes contact; first_order=True:
    the point of the first-order analytic cases."""
    first_order = first_order and model in ("pendulum_h04", "three_cart")
    key = ("nominal", model, separated, first_order)
    if key not in _memo:
        so = oracle_system(model)
        if model.startswith("planar_hand"):
            H = orc.PlanarHandOracle
            if separated:
                x = H.pack([0.0, 2.0, 0.0], [-2.5, 0.0], [2.5, 0.0])
            else:
                x0 = H.pack([0.0, 0.35, 0.0], [-np.pi / 4, -np.pi / 4], [np.pi / 4, np.pi / 4])
                x = orc.rollout(orc.PlanarHandOracle(0.1), x0, np.tile(x0[so.indices_u_into_x], (25, 1)))[-1]
            u = x[so.indices_u_into_x].copy()
        elif model == "box_pivot":
            x = orc.BoxPivotOracle.pack([0.0, 0.5, 0.0], [-3.0, 1.5] if separated else [-0.6, 0.3])
            u = x[so.indices_u_into_x].copy()
        else:
            g = np.random.default_rng(5)
            x = 0.2 * g.normal(size=so.dim_x)
            u = 0.3 + 0.2 * g.normal(size=so.dim_u)
            if model == "bicycle":
                x[3] = 1.0                                              # rolling
            if model == "three_cart":
                x[:3] += [-1.0, 0.0, 1.0]                               # apart: no sample in range makes them touch
            # first-order: a point where the Jacobian differs from sample to sample, or swapped samples cannot be seen
            if model == "pendulum_h04" and first_order:
                x[0] = 1.2                                              # d w'/d theta ~ cos(theta): steep here
            if model == "three_cart" and first_order:
                x[:3] = [-0.2, 0.0, 1.0]                                # carts 1, 2 at touching distance: the sample
                                                                        # decides the branch; cart 3 stays free
        _memo[key] = (x, u)
    x, u = _memo[key]
    return np.tile(x, (T + 1, 1)), np.tile(u, (T, 1))


def perturbations(case, geom, seed=0):
    """The dyadic integers of a case (T, N, nz) and the f32 (dx, du) the launch is given (dx None in the u-only modes).
    `geom`: the geometry of the supplied-sample launch -- its boundary samples are made strong, and one whose squares
    equal those of the row a clamped lane would load instead could be swapped for it unseen, and is redrawn."""
    _, n, m, contact = MODELS[case["model"]]
    u_only = case["mode"] == ZERO_ORDER_B or (case["mode"] == FIRST_ORDER and contact)
    g = np.random.default_rng(7919 * case["T"] + case["N"] + seed)
    k = dyadic_samples(case["T"], case["N"], m if u_only else n + m, g)
    own = owners(geom, case["N"])
    bs = boundary_samples(geom, case["N"], own)

    def strong(count):
        return g.choice([3, 4], size=(count, k.shape[2])) * g.choice([-1, 1], size=(count, k.shape[2]))

    # boundary samples are strong ones, |k| in {3, 4} throughout: the weakest of them sets how tightly the inexact
    # statistics must be compared (ZDF_BOUND below), and a row of single 2^-5 entries would ask for more than f32 gives
    k[:, bs] = strong(k.shape[0] * bs.size).reshape(k.shape[0], bs.size, -1)
    antipodal = case["mode"] == FIRST_ORDER and not contact
    for s in bs:
        c = clamp_row(geom, case["N"], own, s)
        if antipodal and c != s:
            # sums of Jacobians see a swapped sample only through the difference of two Jacobians: make it large --
            # every component of s has the other sign and the other magnitude of the clamped row's
            k[:, s] = -np.sign(k[:, c]) * (7 - np.abs(k[:, c]))
        while c != s:
            same = (k[:, s] ** 2 == k[:, c] ** 2).all(axis=1)
            if not same.any():
                break
            k[same, s] = strong(int(same.sum()))
    z = as_f32(k)
    return (k, None, z) if u_only else (k, np.ascontiguousarray(z[:, :, :n]), np.ascontiguousarray(z[:, :, n:]))


def zero_order_terms(case, x, u, z, weights=None):
    """f64 statistics of ONE timestep of a zero-order mode in the layout of `sums`, from the perturbed columns z (N, nz)
    given in f64: [Gram | z df' | sum z (contact)], df measured from f(x, u) (analytic) or the f32-rounded x."""
    _, n, m, contact = MODELS[case["model"]]
    so = oracle_system(case["model"])
    lay = sums_layout(n, m, case["mode"], contact)
    full = np.zeros((z.shape[0], n + m))
    full[:, lay["z0"]:] = z
    ref = x.astype(np.float32).astype(np.float64) if contact else so.dynamics(x, u)
    df = so.dynamics_batch(x + full[:, :n], u + full[:, n:]) - ref
    w = np.ones(z.shape[0]) if weights is None else weights
    iu = np.triu_indices(lay["nz"])
    out = [((z * w[:, None]).T @ z)[iu], ((z * w[:, None]).T @ df).ravel()]
    if contact:
        out.append((z * w[:, None]).sum(0))
    return np.concatenate(out)


def weakest_mutation(case, geom, ts=(0,)):
    """Over the boundary samples of the geometry and the three faults (dropped, read twice, replaced by the clamped
    row): (every fault changes the exact blocks?, the smallest relative change of the z df' block).  Relative: max
    abs change over the block's max abs value -- the measure the device comparison uses."""
    _, n, m, contact = MODELS[case["model"]]
    lay = sums_layout(n, m, case["mode"], contact)
    N = case["N"]
    own = owners(geom, N)
    k, _, _ = perturbations(case, geom)
    x_trj, u_trj = nominal(case["model"], case["T"])
    bs = boundary_samples(geom, N, own)
    seen, weakest = True, np.inf
    for t in ts:
        z = k[t] * 2.0 ** -5
        base = zero_order_terms(case, x_trj[t], u_trj[t], z)
        scale = np.abs(base[lay["zdf"]]).max()
        rows = np.unique(np.concatenate([bs, [clamp_row(geom, N, own, s) for s in bs]]))
        one = {int(s): zero_order_terms(case, x_trj[t], u_trj[t], z[s:s + 1]) for s in rows}
        for s in bs:
            c = clamp_row(geom, N, own, s)
            for delta in (one[int(s)], one[int(c)] - one[int(s)]) if c != s else (one[int(s)],):
                exact = np.concatenate([delta[lay["gram"]]] + ([delta[lay["sumz"]]] if contact else []))
                seen = seen and bool(np.any(exact != 0))
                weakest = min(weakest, np.abs(delta[lay["zdf"]]).max() / scale)
    return seen, weakest


def weakest_jacobian_swap(case, geom, ts=(0,)):
    """First-order analytic cases: over the boundary samples, the smallest change that replacing the sample by the
    clamped row makes in the f64 sum of Jacobians, relative to the block's max abs value (dropped and doubled samples
    are counted exactly by the structural ones).  Returns (boundary samples whose swap changes anything, that
    minimum).  A swap between two samples with the SAME Jacobian (three carts on one branch) changes nothing in exact
    arithmetic: there is nothing to see, and it is not counted."""
    _, n, m, _ = MODELS[case["model"]]
    so = oracle_system(case["model"])
    N = case["N"]
    own = owners(geom, N)
    k, _, _ = perturbations(case, geom)
    x_trj, u_trj = nominal(case["model"], case["T"], first_order=True)
    bs = boundary_samples(geom, N, own)
    pairs = [(int(s), clamp_row(geom, N, own, s)) for s in bs]
    pairs = [(s, c) for s, c in pairs if s != c]
    visible, weakest = 0, np.inf
    for t in ts:
        z = k[t] * 2.0 ** -5
        scale = np.abs(so.jacobian_xu_batch(x_trj[t] + z[:, :n], u_trj[t] + z[:, n:]).sum(axis=0)).max()
        rows = sorted({r for p in pairs for r in p})
        J = dict(zip(rows, so.jacobian_xu_batch(x_trj[t] + z[rows, :n], u_trj[t] + z[rows, n:]))) if rows else {}
        for s, c in pairs:
            e = np.abs(J[c] - J[s]).max() / scale
            if e > 1e-9:                                               # (the three carts' oracle differentiates numerically)
                visible += 1
                weakest = min(weakest, e)
    return len(pairs) * len(ts), visible, weakest


# ------------------------------------------------------------------------------------------------ the bounds
# Device against the f64 oracle, per kernel family, as max abs deviation over the block's max abs value (z df', the sum
# of Jacobians) or max abs deviation (fitted A, B): 4 x the largest figure measured on an MI355X over the family's
# cases (the measured figure beside it).  tests/test_smooth_geometry_cpu.py keeps every ZDF and JAC bound below a tenth
# of the smallest change a faulty boundary sample makes in the same measure.
ZDF_BOUND = {LIGHT: 1.8e-6,        # measured 4.31e-7 (pendulum zero-order-B, T=3 N=1025)
             (LIGHT, ZERO_ORDER_AB): 1.0e-6,       # 2.51e-7 (pendulum zero-order-AB; 7e-8 from N = 4096 on)
             HEAVY: 4.8e-7,        # 1.20e-7 (bicycle)
             GRAM: 1.6e-5,         # 4.07e-6 (planar hand zero-order-AB, T=2 N=64: state perturbations of 1/8 at a grasp)
             WAVE_DEALT: 2.5e-6,   # 6.11e-7 (box pivoting)
             PARKED: 1.1e-6,       # 2.72e-7 (planar hand under IRS_UG=0)
             UG: 4.8e-6}           # 1.21e-6 (planar hand)
# N = 1: one lane's f32 step against the oracle, nothing averages (and one sample is the whole block: any fault changes it
# by its full size)
ZDF_BOUND_ONE = {LIGHT: 8.1e-6,    # 2.03e-6 (pendulum zero-order-B: df = h du / (m l^2), the difference of two f32 steps)
                 HEAVY: 1.7e-6,    # 4.12e-7
                 GRAM: 1.4e-5,     # 3.39e-6 (planar hand; quadrotor 2.09e-7)
                 WAVE_DEALT: 3.1e-6,   # 7.77e-7
                 PARKED: 4.3e-6,   # 1.07e-6
                 UG: 3.9e-6}       # 9.71e-7
FIT_BOUND = {LIGHT: 1.0e-6,        # 2.61e-7
             HEAVY: 6.4e-7,        # 1.59e-7
             GRAM: 5.6e-6,         # 1.40e-6
             WAVE_DEALT: 2.3e-6,   # 5.80e-7
             PARKED: 5.0e-7,       # 1.24e-7
             UG: 5.3e-6}           # 1.33e-6
# (LIGHT: 4 x measured would be 8.4e-7; a tenth of what one swapped sample changes at T=30 N=20000, 4.04e-6, allows less)
JAC_BOUND = {LIGHT: 4.0e-7,        # 2.09e-7 (pendulum with h = 0.4, T=3 N=16384)
             HEAVY: 4.0e-7}        # 9.90e-8 (quadrotor, T=2 N=1)


def zdf_bound(family, mode, N):
    return ZDF_BOUND_ONE[family] if N == 1 else ZDF_BOUND.get((family, mode), ZDF_BOUND[family])
