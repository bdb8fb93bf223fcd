"""Admission of the any-size bounded TV-LQR cases (tests/helpers/box_values_cases.py) that
tests/test_box_values_gpu.py runs on csrc/boxqp_values.hip, and the host side of its C ABI: the size queries and every
argument error, which are decided without a GPU.

A case is admitted the way tests/test_boxqp_cases_cpu.py admits the compiled sizes' cases: the oracle's ADMM converges
under the cap of 40000 iterations at eps 1e-10 at the recorded rho (the fastest of 1, 10, 100); its solution passes the
solver-independent KKT certificate at 1e-7; of every kind of bound the case declares at least one entry is active; and
each applicable row-handling mutation (shifted rows, swapped sides, row 0 throughout) moves the oracle's solution by more
than 1e-4 -- 1000 x the 1e-7 the device test allows (where the mutated rows contradict each other the mutated ADMM
stops at its cap of 10000, far from the true solution).
"""
import ctypes

import numpy as np
import pytest

from oracle import boxqp_cases as bc
from tests.helpers import box_values_cases as vc


@pytest.mark.parametrize("cid", list(vc.CASES))
def test_case_is_admitted(cid):
    c = vc.case(cid)
    n, m, shape, T = vc.CASES[cid]
    assert (c["At"].shape, c["Bt"].shape, c["idx"]) == ((T, n, n), (T, n, m), None)
    for k in bc.ROW_KEYS:
        assert c[k].shape == ((T + 1, n) if k[0] == "x" else (T, m)), k
    best, its = bc.pick_rho(c)
    assert its[c["rho"]] == its[best], (c["rho"], its)
    x, u, it = vc.reference(cid)
    assert it == its[c["rho"]] and it < 40000, it
    res = bc.kkt(c, x, u)
    assert max(res) <= 1e-7, res
    act, fin = bc.active(c, x, u)
    for group in c["declared"]:
        assert any(act[k][t, j] for k, t, j in group), ("declared bound not active", group[0])
    dist = {}
    for name, rows in bc.mutated_rows(c).items():
        xm, um, itm = bc.solve(c, rows=rows, max_iter=10000, eps=1e-8)
        # (a mutated problem may be infeasible -- on a scalar system a shifted x row and a u row can contradict each
        # other -- and its ADMM then stops at the cap: a kernel with that error reports failure, and the distance
        # below is that of the iterate it stopped at)
        dist[name] = max(np.abs(xm - x).max(), np.abs(um - u).max())
    print("%-10s rho %5.0f  it %5d  KKT %.1e  active %s  mutations %s" % (
        cid, c["rho"], it, max(res), " ".join("%s %d/%d" % (k, act[k].sum(), fin[k].sum()) for k in bc.ROW_KEYS if fin[k].any()),
        " ".join("%s %.1e" % kv for kv in dist.items())))
    for name, d in dist.items():
        assert d > 1e-4, (name, d)


def test_seed_words_are_the_first_at_which_every_declared_kind_binds():
    """Seed word 0 unless the table says otherwise; a recorded word is the first that admits the case: at every
    earlier one a declared kind of bound does not bind, or an applicable mutation leaves the solution where it is."""
    assert set(vc.SEED) <= set(vc.CASES) and set(vc.RHO) == set(vc.CASES)
    for cid, word in vc.SEED.items():
        n, m, shape, T = vc.CASES[cid]
        for earlier in range(word):
            c = vc.build(n, m, shape, T, earlier)
            c["rho"] = bc.pick_rho(c)[0]
            x, u, _ = bc.solve(c)
            seen = True
            for rows in bc.mutated_rows(c).values():
                xm, um, _ = bc.solve(c, rows=rows, max_iter=10000, eps=1e-8)
                seen = seen and max(np.abs(xm - x).max(), np.abs(um - u).max()) > 1e-4
            assert not (vc.all_declared_bind(c, x, u) and seen), (cid, earlier)


def test_sizes_and_horizons_cover_the_kernel():
    assert set(vc.SIZES) == {(1, 1), (3, 2), (9, 5), (17, 9), (32, 16), (32, 1), (1, 16)}
    ran = {}
    for n, m, shape, T in vc.CASES.values():
        ran.setdefault((n, m), set()).add((shape, T))
    for size in vc.SIZES:
        want = {("B1", 12), ("B2", 12), ("B3", 12)}
        if size == (1, 1):
            want |= {("B5u", 1), ("B5x", 1), ("B5", 2)}
        assert ran[size] == want, (size, ran[size])


def test_linear_system_is_the_linear_model():
    c = vc.case("s3x2-B2")
    plant = vc.LinearSystem(c["At"], c["Bt"], c["ct"])
    x = c["x0"]
    for t in range(c["T"]):
        x = plant.dynamics(x, c["us"][t])
        np.testing.assert_allclose(x, c["At"][t] @ c["xs"][t] + c["Bt"][t] @ c["us"][t] + c["ct"][t], rtol=0, atol=1e-9)


def test_descent_problems_bind_and_converge_on_the_oracle():
    """The descents tests/test_box_values_gpu.py runs, on the oracle alone: every tail converges under the cap, the u
    bound is active, and (cart-pole, on the oracle's own linearisation) the velocity bound too."""
    for cid in vc.RESUMED:
        (x_lo, x_hi, u_lo, u_hi), xo, uo, iters = vc.resumed_reference(cid)
        assert max(iters) < vc.QP["max_iter"], (cid, iters)
        assert min(np.abs(uo - u_lo).min(), np.abs(uo - u_hi).min()) < 1e-9, cid
        assert min(np.abs(xo[1:] - x_lo).min(), np.abs(xo[1:] - x_hi).min()) < 1e-7, cid
    b = vc.cartpole_bounds()
    vel = vc.CARTPOLE_VELOCITY
    xo, uo, iters = vc.cartpole_bounded_descent(*b["lin"])
    assert max(iters) < vc.QP["max_iter"], iters
    assert np.abs(uo).max() == pytest.approx(b["uhi"][0], abs=1e-9)
    assert np.abs(xo[:, vel]).max() > b["xhi"][vel] - 1e-3
    assert np.abs(uo - b["un"]).max() > 1e-2


# ------------------------------------------------------------------------------------------------ the C ABI, no GPU
@pytest.fixture(scope="module")
def lib():
    from irs_mpc_amd import _lib
    return _lib.load()


def test_exports(lib):
    import irs_mpc_amd
    from irs_mpc_amd import _lib, device as dev
    for name in ("irs_box_values_workspace_bytes", "irs_box_values_horizon_limit", "irs_box_values_lds_bytes",
                 "irs_box_values_begin", "irs_box_values_tail"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    for name in ("box_values_begin", "box_values_tail", "box_values_solve", "box_values_horizon_limit"):
        assert callable(getattr(dev, name)), name
    assert irs_mpc_amd.IrsLqrParameters().qp_model_free is False
    assert callable(irs_mpc_amd.torch_system.TorchDeviceModel.tvlqr_box_descent)


def test_workspace_bytes_are_positive_and_monotone(lib):
    f = lib.irs_box_values_workspace_bytes
    for n, m, T in [(1, 1, 1), (3, 2, 12), (12, 4, 200), (32, 16, 16)]:
        assert f(n, m, T) > 0 and f(n, m, T) % 256 == 0
    for m in (1, 5, 16):
        for T in (1, 12, 50):
            v = [f(n, m, T) for n in range(1, 33)]
            assert all(a <= b for a, b in zip(v, v[1:])), ("n", m, T)
    for n in (1, 9, 32):
        for T in (1, 12, 50):
            v = [f(n, m, T) for m in range(1, 17)]
            assert all(a <= b for a, b in zip(v, v[1:])), ("m", n, T)
        for m in (1, 16):
            v = [f(n, m, T) for T in range(1, 70)]
            assert all(a <= b for a, b in zip(v, v[1:])), ("T", n, m)
    assert f(0, 1, 5) == 0 and f(33, 1, 5) == 0 and f(4, 17, 5) == 0 and f(4, 1, 0) == 0


def test_horizon_limit(lib):
    lim = lib.irs_box_values_horizon_limit
    assert lim(12, 4) >= 200                                  # the quadrotor script's horizon
    for n in range(1, 33):
        for m in range(1, 17):
            L = lim(n, m)
            assert L >= 16, (n, m, L)
            # the planner the launch reads: LDS within the budget up to the limit, beyond it one step later
            assert lib.irs_box_values_lds_bytes(n, m, L) <= 160 * 1024 - 512 < lib.irs_box_values_lds_bytes(n, m, L + 1)
    assert lim(0, 1) == 0 and lim(33, 1) == 0 and lim(1, 0) == 0 and lim(1, 17) == 0


def _call(n=3, m=2, T=12, **kw):
    from irs_mpc_amd import _lib
    one = 4096        # any non-null, 256-byte aligned address: validation happens before anything is dereferenced
    f = dict(n=n, m=m, T=T, At=one, Bt=one, ct=one, Q=one, Qd=one, R=one, alpha_R=0.5, xd_trj=one, x_lo=None, x_hi=None,
             x_rows=1, u_lo=one, u_hi=one, u_rows=1, rho=10.0, relax=1.6, workspace=one, workspace_bytes=1 << 30, info=one)
    f.update(kw)
    return _lib.BoxValuesCall(**f)


def test_argument_errors_without_gpu(lib):
    from irs_mpc_amd import _lib
    one = 4096
    INV, UNS, WSP = _lib.IRS_ERR_INVALID_ARG, _lib.IRS_ERR_UNSUPPORTED, _lib.IRS_ERR_WORKSPACE
    need = lib.irs_box_values_workspace_bytes(3, 2, 12)
    too_long = lib.irs_box_values_horizon_limit(3, 2) + 1
    bad = [(dict(n=0), INV, b"1<=n<=32"), (dict(n=33), INV, b"1<=n<=32"), (dict(m=0), INV, b"1<=m<=16"),
           (dict(m=17), INV, b"1<=m<=16"), (dict(T=0), INV, b"T>=1"),
           (dict(T=too_long), UNS, b"limit T <= %d" % (too_long - 1)),
           (dict(At=None), INV, b"null"), (dict(Bt=None), INV, b"null"), (dict(ct=None), INV, b"null"),
           (dict(Q=None), INV, b"null"), (dict(Qd=None), INV, b"null"), (dict(R=None), INV, b"null"),
           (dict(xd_trj=None), INV, b"null"), (dict(info=None), INV, b"null"),
           (dict(u_rows=5), INV, b"u_rows"), (dict(x_lo=one, x_rows=12), INV, b"x_rows"),
           (dict(rho=0.0), INV, b"rho"), (dict(rho=-1.0), INV, b"rho"), (dict(relax=0.0), INV, b"relax"),
           (dict(relax=2.0), INV, b"relax"),
           (dict(workspace=None), WSP, b"workspace"), (dict(workspace_bytes=need - 1), WSP, b"workspace"),
           (dict(workspace=one + 8), WSP, b"aligned")]
    for kw, code, word in bad:
        c = _call(**kw)
        assert lib.irs_box_values_begin(ctypes.byref(c), None) == code, kw
        assert word in lib.irs_last_error(), (kw, lib.irs_last_error())
        assert lib.irs_box_values_tail(ctypes.byref(c), 0, one, 100, 1e-8, one, None, None, None) == code, kw
        assert word in lib.irs_last_error(), (kw, lib.irs_last_error())
    assert lib.irs_box_values_begin(None, None) == INV
    # the tail's own arguments
    c = _call()
    for args, word in [((-1, one, 100, 1e-8, one), b"0 <= t < T"), ((12, one, 100, 1e-8, one), b"0 <= t < T"),
                       ((0, None, 100, 1e-8, one), b"null"), ((0, one, 100, 1e-8, None), b"null"),
                       ((0, one, 0, 1e-8, one), b"max_iter"), ((0, one, 100, 0.0, one), b"eps")]:
        assert lib.irs_box_values_tail(ctypes.byref(c), *args, None, None, None) == INV, args
        assert word in lib.irs_last_error(), (args, lib.irs_last_error())
