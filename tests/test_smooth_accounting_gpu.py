"""Every sample counted exactly once, on every launch geometry of the sample pass (csrc/smooth.hip, csrc/smooth_ug.hip).

The cases of oracle/smooth_cases.py -- admitted by tests/test_smooth_geometry_cpu.py: each reaches the geometry it
names, and a sample dropped, read twice or replaced by a clamped row at any boundary of that geometry changes the
blocks compared here -- run with samples k 2^-5, integer |k| <= 4, a different draw per timestep.  Their Gram and
sum-of-z statistics are exact in f32 in any summation order, so the device must reproduce the integer answer BIT FOR
BIT; the remaining statistics are held to the f64 oracle within the bounds of oracle/smooth_cases.py (4 x the
deviation measured on an MI355X, which the CPU admission keeps below a tenth of what one faulty sample changes).
Device-drawn samples cannot be dyadic: the launch that draws is compared with the same kernel fed the same draws.
"""
import os

import numpy as np
import pytest
import torch

from oracle import smooth_cases as sc

pytestmark = pytest.mark.gpu

SEED, ITER, OFFSET = 11, 2, 12345          # device draws: a non-zero sample_offset, as a sharded run has


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()     # fails loudly if the HIP library is missing
    return irs_mpc_amd


_dm = {}


def device_model(amd, model):
    if model not in _dm:
        cls, args, kw, _ = sc.SYSTEMS[model]
        _dm[model] = getattr(amd, cls)(*args, **kw).dm()
    return _dm[model]


def call(case, fn, *a, **kw):
    """One library call; the planar hand's general kernels are selected per call (IRS_UG is read per call)."""
    if not sc.needs_general_kernel(case):
        return fn(*a, **kw)
    before = os.environ.get("IRS_UG")
    os.environ["IRS_UG"] = "0"
    try:
        return fn(*a, **kw)
    finally:
        if before is None:
            os.environ.pop("IRS_UG", None)
        else:
            os.environ["IRS_UG"] = before


def setup(amd, case, separated=False, first_order=False):
    from irs_mpc_amd import device as dev
    dm = device_model(amd, case["model"])
    x_trj, u_trj = sc.nominal(case["model"], case["T"], separated, first_order)
    geom = {src: call(case, dm.smooth_geometry, case["mode"], case["T"], case["N"], src == "r")
            for src in case["sources"]}
    for g in geom.values():
        assert sc.admit(case, g, case["N"]) is None, (sc.admit(case, g, case["N"]), g)
    return dm, x_trj, u_trj, dev.to_dev(x_trj), dev.to_dev(u_trj), geom


def f32dev(a):
    from irs_mpc_amd import device as dev
    return None if a is None else dev.to_dev(a, dev.F32)


def rel(got, want):
    """max abs deviation over the block's max abs value."""
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def some_steps(T):
    return sorted({0, T // 2, T - 1})


def fit_from(case, x, u, terms):
    """(A or None, B) of one timestep from f64 statistics in the layout of `sums`: the solve of the normal equations."""
    _, n, m, contact = sc.MODELS[case["model"]]
    lay = sc.sums_layout(n, m, case["mode"], contact)
    nz = lay["nz"]
    G = np.zeros((nz, nz))
    G[np.triu_indices(nz)] = terms[lay["gram"]]
    G = G + np.triu(G, 1).T
    H = terms[lay["zdf"]].reshape(nz, n).copy()
    if contact:
        so = sc.oracle_system(case["model"])
        H -= np.outer(terms[lay["sumz"]], so.dynamics(x, u) - x.astype(np.float32).astype(np.float64))
    AB = np.linalg.solve(G, H).T
    return (AB[:, :n], AB[:, n:]) if case["mode"] == sc.ZERO_ORDER_AB else (None, AB)


def free_rows(case):
    _, n, m, contact = sc.MODELS[case["model"]]
    if not contact:
        return np.arange(n)
    return np.setdiff1d(np.arange(n), sc.oracle_system(case["model"]).indices_u_into_x)


ZERO_S = [cid for cid, c in sc.CASES.items() if c["mode"] != sc.FIRST_ORDER and "s" in c["sources"]]
ZERO_R = [cid for cid, c in sc.CASES.items() if c["mode"] != sc.FIRST_ORDER and "r" in c["sources"]]
FIRST_ANALYTIC = [cid for cid, c in sc.CASES.items() if c["mode"] == sc.FIRST_ORDER and not sc.MODELS[c["model"]][3]]
FIRST_CONTACT = [cid for cid, c in sc.CASES.items() if c["mode"] == sc.FIRST_ORDER and sc.MODELS[c["model"]][3]]


@pytest.mark.parametrize("cid", ZERO_S)
def test_zero_order_supplied_samples_counted_once(amd, cid):
    """Gram and sum z == the integer answer, bit for bit, from the two-stage launch and from the fused one; z df' and
    the fitted (A, B, c) against the f64 oracle.  The planar hand runs at its settled grasp, where Gaussian commands
    of 0.3 rad park 8-40 % of the samples; what share these smaller dyadic commands park was not counted, so for the
    rings this is the exact count of whatever is parked, and test_first_order_parked_samples_finished_exactly_once
    below is the test that runs at the measured noise."""
    c = sc.CASES[cid]
    _, n, m, contact = sc.MODELS[c["model"]]
    dm, x_trj, u_trj, xd, ud, geom = setup(amd, c)
    k, dx, du = sc.perturbations(c, geom["s"])
    dxd, dud = f32dev(dx), f32dev(du)
    sums = call(c, dm.smooth_accumulate, c["mode"], xd, ud, dxd, dud).cpu().numpy()
    fused = call(c, dm.smooth, c["mode"], xd, ud, dxd, dud)
    fsums = fused["sums"].cpu().numpy()
    lay = sc.sums_layout(n, m, c["mode"], contact)
    G, S = sc.exact_blocks(k)
    np.testing.assert_array_equal(sums[:, lay["gram"]], G)
    np.testing.assert_array_equal(fsums[:, lay["gram"]], G)
    if contact:
        np.testing.assert_array_equal(sums[:, lay["sumz"]], S)
        np.testing.assert_array_equal(fsums[:, lay["sumz"]], S)
    fam = geom["s"]["family"]
    worst, worst_fit = 0.0, 0.0
    Bt, At, ct = fused["Bt"].cpu().numpy(), fused["At"].cpu().numpy(), fused["ct"].cpu().numpy()
    so = sc.oracle_system(c["model"])
    rows = free_rows(c)
    for t in some_steps(c["T"]):
        want = sc.zero_order_terms(c, x_trj[t], u_trj[t], k[t] * 2.0 ** -5)
        worst = max(worst, rel(sums[t, lay["zdf"]], want[lay["zdf"]]), rel(fsums[t, lay["zdf"]], want[lay["zdf"]]))
        if c["N"] >= 8 * lay["nz"]:
            A, B = fit_from(c, x_trj[t], u_trj[t], want)
            worst_fit = max(worst_fit, float(np.abs(Bt[t][rows] - B[rows]).max()))
            if not contact:
                # analytic models: all of (A, B, c); A of the u-only mode is the exact linearisation.  (Contact models
                # return the DECOUPLED pair: their A and the actuated rows of B are fixed by the structure, not fitted)
                A = so.jacobian_xu(x_trj[t], u_trj[t])[:, :n] if A is None else A
                worst_fit = max(worst_fit, float(np.abs(At[t] - A).max()))
                cw = so.dynamics(x_trj[t], u_trj[t]) - A.dot(x_trj[t]) - B.dot(u_trj[t])
                worst_fit = max(worst_fit, float(np.abs(ct[t] - cw).max()))
    print("%s [%s]: z df' off the f64 oracle by %.3g of the block (bound %.3g); fitted A, B, c by %.3g (bound %.3g)" % (
        cid, fam, worst, sc.zdf_bound(fam, c["mode"], c["N"]), worst_fit, sc.FIT_BOUND[fam]))
    assert worst <= sc.zdf_bound(fam, c["mode"], c["N"])
    assert worst_fit <= sc.FIT_BOUND[fam]
    if c["N"] >= 8 * lay["nz"]:
        assert int(fused["info"].abs().sum().item()) == 0


@pytest.mark.parametrize("cid", ZERO_R)
def test_zero_order_device_drawn_samples_counted_once(amd, cid):
    """The launch that draws its samples == the same kernel fed those draws (irs_rng_samples: same seed, iteration and
    a non-zero sample offset) == the f64 Gram of the draws.  rtol 1e-5 + atol 1e-6 max|sums|: what the suite gives two
    instantiations of one template; a lost boundary sample moves the Gram by at least ten times that.
    Measured on an MI355X: drawn vs supplied at most 0.44 of that tolerance (planar hand zero-order-AB, N = 3), the
    Gram vs f64 0.028 of it; the weakest boundary sample of any case moves the Gram by 54 tolerances."""
    c = sc.CASES[cid]
    _, n, m, contact = sc.MODELS[c["model"]]
    dm, x_trj, u_trj, xd, ud, geom = setup(amd, c)
    u_only = c["mode"] == sc.ZERO_ORDER_B
    su, sx = np.full(m, 0.1), np.full(n, 0.0 if u_only else 0.05)
    lay = sc.sums_layout(n, m, c["mode"], contact)
    iu = np.triu_indices(lay["nz"])
    own = sc.owners(geom["r"], c["N"], True)
    bs = sc.boundary_samples(geom["r"], c["N"], own)
    worst, worstG, effect = 0.0, 0.0, np.zeros(bs.size)
    # which lane reads sample s does not depend on the timestep or on the draw: a fault at s shows in the launch if it
    # shows at ANY timestep, so short horizons are run on several iterations' draws until there are eight of them
    for it in range(ITER, ITER + max(1, -(-8 // c["T"]))):
        dxd, dud = dm.rng_samples(c["T"], c["N"], sx, su, SEED, it, OFFSET)
        a = call(c, dm.smooth_accumulate_rng, c["mode"], xd, ud, c["N"], None if u_only else sx, su, SEED, it,
                 OFFSET).cpu().numpy()
        b = call(c, dm.smooth_accumulate, c["mode"], xd, ud, None if u_only else dxd, dud).cpu().numpy()
        z = np.concatenate([dxd.cpu().numpy(), dud.cpu().numpy()], axis=2).astype(np.float64)[:, :, lay["z0"]:]
        G = np.einsum("tni,tnj->tij", z, z)[:, iu[0], iu[1]]
        scale = np.abs(b).max()        # as test_fused_launch_equals_two_stage (tests/test_gpu_parity.py): of the whole tensor
        for name in ("gram", "zdf", "sumz"):
            if lay[name] is None:
                continue
            tol = 1e-5 * np.abs(b[:, lay[name]]) + 1e-6 * scale
            worst = max(worst, float((np.abs(a[:, lay[name]] - b[:, lay[name]]) / tol).max()))
        tolG = 1e-5 * np.abs(G) + 1e-6 * scale
        worstG = max(worstG, float((np.abs(a[:, lay["gram"]] - G) / tolG).max()))
        # admission: how many tolerances the loss of boundary sample s moves the Gram
        e = (np.einsum("tni,tnj->tnij", z[:, bs], z[:, bs])[:, :, iu[0], iu[1]] / tolG[:, None, :]).max(axis=2)
        effect = np.maximum(effect, e.max(axis=0))
    print("%s [%s]: drawn vs supplied %.3g tolerances, Gram vs f64 %.3g tolerances; the weakest boundary sample moves "
          "the Gram by %.3g tolerances" % (cid, geom["r"]["family"], worst, worstG, effect.min()))
    assert worst <= 1.0
    assert worstG <= 1.0
    assert effect.min() >= 10.0


@pytest.mark.parametrize("cid", FIRST_ANALYTIC)
def test_first_order_analytic_samples_counted_once(amd, cid):
    """The sum of the sampled Jacobians: its structurally constant entries (d p'/d p = 1, the pendulum's d w'/d w) must
    be N exactly -- for the quadrotor that is the compact-Jacobian path's sample counter -- the rest against the f64
    oracle; device-drawn samples against the same kernel fed the draws."""
    c = sc.CASES[cid]
    _, n, m, _ = sc.MODELS[c["model"]]
    so = sc.oracle_system(c["model"])
    dm, x_trj, u_trj, xd, ud, geom = setup(amd, c, first_order=True)
    g = np.random.default_rng(3)
    Jp = so.jacobian_xu_batch(x_trj[0] + g.uniform(-0.125, 0.125, size=(32, n)),
                              u_trj[0] + g.uniform(-0.125, 0.125, size=(32, m)))
    # (1e-6: the three carts' oracle differentiates by central differences)
    ones = np.flatnonzero((np.abs(Jp - 1.0) < 1e-6).all(axis=0).ravel() & np.eye(n, n + m, dtype=bool).ravel())
    assert ones.size >= 1
    if "s" in c["sources"]:
        k, dx, du = sc.perturbations(c, geom["s"])
        sums = dm.smooth_accumulate(c["mode"], xd, ud, f32dev(dx), f32dev(du)).cpu().numpy()
        np.testing.assert_array_equal(sums[:, ones], float(c["N"]))
        worst = 0.0
        for t in some_steps(c["T"]):
            z = k[t] * 2.0 ** -5
            want = so.jacobian_xu_batch(x_trj[t] + z[:, :n], u_trj[t] + z[:, n:]).sum(axis=0).ravel()
            worst = max(worst, rel(sums[t], want))
        fam = geom["s"]["family"]
        print("%s [%s]: sum of Jacobians off the f64 oracle by %.3g of the block (bound %.3g)" % (
            cid, fam, worst, sc.JAC_BOUND[fam]))
        assert worst <= sc.JAC_BOUND[fam]
    if "r" in c["sources"]:
        sx, su = np.full(n, 0.05), np.full(m, 0.1)
        dxd, dud = dm.rng_samples(c["T"], c["N"], sx, su, SEED, ITER, OFFSET)
        a = dm.smooth_accumulate_rng(c["mode"], xd, ud, c["N"], sx, su, SEED, ITER, OFFSET).cpu().numpy()
        b = dm.smooth_accumulate(c["mode"], xd, ud, dxd, dud).cpu().numpy()
        np.testing.assert_array_equal(a[:, ones], float(c["N"]))
        tol = 1e-5 * np.abs(b) + 1e-6 * np.abs(b).max(axis=1, keepdims=True)
        print("%s: drawn vs supplied %.3g tolerances" % (cid, float((np.abs(a - b) / tol).max())))
        assert (np.abs(a - b) <= tol).all()


_b64 = {}


@pytest.mark.parametrize("cid", FIRST_CONTACT)
def test_first_order_contact_samples_counted_once(amd, cid):
    """Where no command in range makes contact every sample has the same derivative: with all-zero du the mean B of N
    samples must be that of the 64-sample launch of the same kernel, to the f32 bound for summing equal addends,
    (trips per lane + 10) 2^-24 relative -- a tenth of 1 / N, what one lost sample changes (admission).  Device-drawn
    commands at that pose: the same B.  Measured on an MI355X: equal bit for bit in every case."""
    c = sc.CASES[cid]
    _, n, m, _ = sc.MODELS[c["model"]]
    dm, x_trj, u_trj, xd, ud, geom = setup(amd, c, separated=True)
    key = (c["model"], c["T"], sc.needs_general_kernel(c))
    if key not in _b64:
        o = call(c, dm.smooth, c["mode"], xd, ud, None, f32dev(np.zeros((c["T"], 64, m), np.float32)))
        _b64[key] = o["Bt"].cpu().numpy().copy()
    B64 = _b64[key]
    assert np.abs(B64).max() > 0.5          # the actuated rows follow the command
    o = call(c, dm.smooth, c["mode"], xd, ud, None, f32dev(np.zeros((c["T"], c["N"], m), np.float32)))
    B = o["Bt"].cpu().numpy()
    bound = (sc.trips_per_lane(geom["s"], c["N"]) + 10) * 2.0 ** -24
    err = np.abs(B - B64)
    print("%s [%s]: B of N = %d vs N = 64 off by %.3g relative (bound %.3g)" % (
        cid, geom["s"]["family"], c["N"], float((err / np.maximum(np.abs(B64), 1e-300))[B64 != 0].max()), bound))
    assert (err <= bound * np.abs(B64)).all()
    o2 = call(c, dm.smooth_rng, c["mode"], xd, ud, c["N"], None, np.full(m, 0.05), SEED, ITER)
    B2 = o2["Bt"].cpu().numpy()
    bound2 = (sc.trips_per_lane(geom["r"], c["N"], True) + 10) * 2.0 ** -24
    assert (np.abs(B2 - B64) <= bound2 * np.abs(B64)).all()


PARKED_FIRST = [cid for cid in FIRST_CONTACT if sc.CASES[cid]["model"] == "planar_hand" and sc.CASES[cid]["T"] > 1]


@pytest.mark.parametrize("cid", PARKED_FIRST)
def test_first_order_parked_samples_finished_exactly_once(amd, cid):
    """First-order at the settled grasp (8-40 % of the samples parked and finished in flush trips) == the mean of the
    per-sample lanes (irs_contact_samples_f32, the undeferred method), at T > 1: the noise and the 2e-6 of
    test_parked_samples_are_finished_exactly_once (tests/test_gpu_parity.py), which runs T = 1 only.  Measured on
    an MI355X: 2.1e-7 to 3.9e-7 for the uniform-geometry kernel, 1.1e-7 to 1.5e-7 for the general kernel under
    IRS_UG=0 -- no sample changed face, so the 2e-6 holds for both."""
    from irs_mpc_amd import device as dev
    c = sc.CASES[cid]
    _, n, m, _ = sc.MODELS[c["model"]]
    dm, x_trj, u_trj, xd, ud, geom = setup(amd, c)
    T, N = c["T"], c["N"]
    du = (0.3 * np.random.default_rng(11).normal(size=(T, N, m))).astype(np.float32)
    dud = f32dev(du)
    _, Bs, _ = dm.contact_samples_f32(dev.to_dev(x_trj[0]), dev.to_dev(u_trj[0]), dud.reshape(T * N, m))
    want = Bs.cpu().numpy().astype(np.float64).reshape(T, N, n, m).mean(axis=1)
    o = call(c, dm.smooth, c["mode"], xd, ud, None, dud)
    rows = free_rows(c)
    err = float(np.abs(o["Bt"].cpu().numpy()[:, rows] - want[:, rows]).max())
    print("%s [%s]: mean B off the per-sample lanes by %.3g (bound 2e-6; one sample on another face: ~%.3g)" % (
        cid, geom["s"]["family"], err, 1.0 / N))
    assert err <= 2e-6
