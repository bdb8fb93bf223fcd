"""CPU-side checks of the device-resident CEM entry points (include/irs_hip.h: irs_cem_candidates,
irs_cem_rollout_costs[_quasistatic]_drawn, irs_cem_refit_drawn, irs_cem_iterate): the symbols exist and are bound, the
scratch query behaves, and every argument error is reported before anything is launched -- no GPU is touched here."""
import ctypes
import os

import pytest

NEW_SYMBOLS = ("irs_cem_candidates", "irs_cem_rollout_costs_drawn", "irs_cem_rollout_costs_quasistatic_drawn",
               "irs_cem_refit_drawn", "irs_cem_iterate", "irs_cem_iterate_scratch_bytes")
INVALID_ARG, UNSUPPORTED = -1, -3
PENDULUM, BOX_PIVOT_EXACT = 0, 9


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from irs_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.load()


def addr(i):
    """Distinct non-null addresses 64 KiB apart: validation happens before anything is dereferenced."""
    return 0x10000 * (i + 1)


def iterate_call(model=PENDULUM, params=(0.05,), T=30, m=1, B=500, n_elite=25, quasistatic=0, **over):
    from irs_mpc_amd import _lib
    lib = _lib.load()
    c = _lib.CemIterateCall()
    c.model, c.n_params = model, len(params)
    for i, v in enumerate(params):
        c.params[i] = v
    c.T, c.B, c.n_elite, c.n_descents, c.quasistatic = T, B, n_elite, 4, quasistatic
    c.seed, c.iter0 = 7, 1
    for i, name in enumerate(("Q", "Qd", "R", "xd_trj", "x0", "u_trj0", "std0", "u_hist", "std_hist", "x_hist",
                              "cost_hist", "scratch")):
        setattr(c, name, addr(i))
    c.scratch_bytes = lib.irs_cem_iterate_scratch_bytes(T, m, B, n_elite)
    for k, v in over.items():
        setattr(c, k, v)
    return c


def test_new_symbols_are_exported_and_bound(lib):
    from irs_mpc_amd import _lib
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), "libirs_hip.so does not export %s" % s
        assert s in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.CemIterateCall) > 0
    from irs_mpc_amd.device import DeviceModel
    for name in ("cem_candidates", "cem_rollout_costs_drawn", "cem_rollout_costs_quasistatic_drawn", "cem_refit_drawn",
                 "cem_iterate"):
        assert callable(getattr(DeviceModel, name))
    assert lib.irs_abi_version() == 1          # entry points are only added


def test_parameter_classes_carry_device_seed():
    import irs_mpc_amd as amd
    assert amd.CemParameters().device_seed is None
    assert amd.CemQuasistaticParameters().device_seed is None


def test_iterate_scratch_bytes(lib):
    q = lib.irs_cem_iterate_scratch_bytes
    assert q(30, 1, 500, 25) > 0 and q(80, 2, 50000, 2500) >= 50000 * 8 + 2500 * 4
    sizes_B = [q(30, 1, B, 5) for B in (5, 6, 64, 300, 5000, 50000)]
    assert sizes_B == sorted(sizes_B) and sizes_B[0] < sizes_B[-1]
    sizes_e = [q(30, 1, 50000, e) for e in (1, 16, 37, 2500, 50000)]
    assert sizes_e == sorted(sizes_e) and sizes_e[0] < sizes_e[-1]
    assert q(0, 1, 500, 25) == 0 and q(30, 1, 0, 25) == 0


def test_refit_drawn_argument_errors(lib):
    mean, std, costs, idx, u_new, std_new = (addr(i) for i in range(6))
    call = lambda *a: lib.irs_cem_refit_drawn(30, 1, 300, *a, None)          # noqa: E731
    # n_elite > B
    assert call(301, mean, std, 7, 1, 0, costs, idx, u_new, std_new) == INVALID_ARG
    # a null output pointer
    assert call(37, mean, std, 7, 1, 0, costs, idx, None, std_new) == INVALID_ARG
    assert call(37, mean, std, 7, 1, 0, costs, idx, u_new, None) == INVALID_ARG
    assert call(37, mean, std, 7, 1, 0, costs, None, u_new, std_new) == INVALID_ARG
    # aliased buffers: the refit reads the old mean / std while it writes the new ones
    assert call(37, mean, std, 7, 1, 0, costs, idx, mean, std_new) == INVALID_ARG
    assert call(37, mean, std, 7, 1, 0, costs, idx, u_new, std) == INVALID_ARG
    assert call(37, mean, std, 7, 1, 0, costs, idx, std, mean) == INVALID_ARG
    assert call(37, mean, std, 7, 1, 0, costs, idx, mean + 8 * 29, std_new) == INVALID_ARG   # partial overlap
    assert b"alias" in lib.irs_last_error()


def test_drawn_rollout_and_candidates_argument_errors(lib):
    from irs_mpc_amd._lib import dbl_array
    p = dbl_array([0.05])
    a = [addr(i) for i in range(8)]
    assert lib.irs_cem_candidates(5, 1, 0, a[0], a[1], 7, 1, 0, a[2], None) == INVALID_ARG
    assert lib.irs_cem_candidates(5, 1, 300, a[0], a[1], 7, 1, 0, None, None) == INVALID_ARG
    assert lib.irs_cem_rollout_costs_drawn(PENDULUM, p, 1, 30, 300, a[0], a[1], 7, 1, 0, a[2], a[3], a[4], a[5], None,
                                           None) == INVALID_ARG
    assert lib.irs_cem_rollout_costs_drawn(PENDULUM, p, 1, 30, 300, None, a[1], 7, 1, 0, a[2], a[3], a[4], a[5], a[6],
                                           None) == INVALID_ARG
    assert lib.irs_cem_rollout_costs_quasistatic_drawn(PENDULUM, p, 1, 30, 300, a[0], a[1], 7, 1, 0, a[2], a[3], a[4],
                                                       a[5], a[6], None, None) == INVALID_ARG


def test_iterate_argument_errors(lib):
    run = lambda c: lib.irs_cem_iterate(ctypes.byref(c), None)               # noqa: E731
    assert lib.irs_cem_iterate(None, None) == INVALID_ARG
    assert run(iterate_call(n_elite=501)) == INVALID_ARG                     # n_elite > B
    for name in ("u_hist", "std_hist", "x_hist", "cost_hist", "scratch"):    # a null output pointer
        assert run(iterate_call(**{name: None})) == INVALID_ARG, name
    assert run(iterate_call(u_trj0=None)) == INVALID_ARG
    c = iterate_call()
    c.scratch_bytes -= 1                                                     # scratch too small
    assert run(c) == INVALID_ARG
    assert b"scratch" in lib.irs_last_error()
    assert run(iterate_call(n_descents=0)) == INVALID_ARG


def test_iterate_quasistatic_needs_a_position_controlled_model(lib):
    assert lib.irs_cem_iterate(ctypes.byref(iterate_call(quasistatic=1)), None) == UNSUPPORTED
    assert b"position controlled" in lib.irs_last_error()
    # ... and, on a position-controlled model, its terminal weight
    box = (0.1, 9.81, 1.0, 0.5, 0.5, 50000.0, 0.1, 50.0)
    c = iterate_call(model=BOX_PIVOT_EXACT, params=box, T=8, m=2, B=200, n_elite=10, quasistatic=1, Qd=None)
    assert lib.irs_cem_iterate(ctypes.byref(c), None) == INVALID_ARG
