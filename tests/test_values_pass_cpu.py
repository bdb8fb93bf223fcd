"""CPU-side checks of the values pass (csrc/smooth_values.hip): its size queries and the argument validation of its
three entries, which is decided before the first HIP call -- no device is touched here."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID_ARG, WORKSPACE = -1, -4
ONE = 4096          # any non-null, 256-byte aligned address: validation happens before anything is dereferenced


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from irs_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.load()


def closed_form(n, m):
    d = n + m
    return d * (d + 1) // 2 + d * n


def test_sums_len_is_the_zero_order_ab_layout(lib):
    from irs_mpc_amd._lib import MODEL_PENDULUM, MODEL_QUADROTOR, SMOOTH_ZERO_ORDER_AB
    assert lib.irs_values_sums_len(2, 1) == lib.irs_sums_len(MODEL_PENDULUM, SMOOTH_ZERO_ORDER_AB) == closed_form(2, 1)
    assert lib.irs_values_sums_len(12, 4) == lib.irs_sums_len(MODEL_QUADROTOR, SMOOTH_ZERO_ORDER_AB) == closed_form(12, 4)
    assert lib.irs_values_sums_len(32, 16) == 48 * 49 // 2 + 48 * 32
    for n, m in ((0, 1), (33, 1), (1, 0), (1, 17)):
        assert lib.irs_values_sums_len(n, m) == INVALID_ARG
        assert lib.irs_last_error() != b""


def test_workspace_bytes_positive_and_monotone(lib):
    for n, m in ((2, 1), (12, 4), (32, 16)):
        prev = 0
        for T in (1, 2, 3, 30, 50, 200, 1024):
            b = lib.irs_smooth_values_workspace_bytes(n, m, T, 10000)
            assert b > 0 and b >= prev, (n, m, T, b, prev)
            prev = b
        prev = 0
        for N in (1, 63, 64, 255, 256, 257, 1000, 10000, 100000, 1000000):
            b = lib.irs_smooth_values_workspace_bytes(n, m, 30, N)
            assert b > 0 and b >= prev, (n, m, N, b, prev)
            prev = b
    # ... densely: every N up to 5000 (and on to 20000 in steps of 7) at several T, every T at several N -- the launch
    # geometry itself saws (nblk is recounted after the chunk is rounded to whole trips: T = 30 has 18 workgroups per
    # timestep at N = 4608 and 14 at N = 10000), so the workspace is sized from a bound that does not; and the
    # partials of the geometry that runs always fit
    out = (ctypes.c_longlong * 4)()
    wsb, P = lib.irs_smooth_values_workspace_bytes, closed_form(5, 2)

    def fits(T, N, b):
        assert lib.irs_smooth_values_geometry(T, N, out) == 0
        return T * out[1] * P * 8 <= b

    Ns = list(range(1, 5001)) + list(range(5001, 20001, 7))
    for T in (1, 2, 3, 13, 14, 30, 50, 171, 512, 1024):
        prev = 0
        for N in Ns:
            b = wsb(5, 2, T, N)
            assert b >= prev and fits(T, N, b), (T, N, b, prev)
            prev = b
    for N in (1, 100, 256, 257, 1000, 4608, 9472, 10000, 100000, 1000000, 2 ** 31 - 1):
        prev = 0
        for T in range(1, 1025):
            b = wsb(5, 2, T, N)
            assert b >= prev and fits(T, N, b), (T, N, b, prev)
            prev = b
    # ... and in n and m
    for n in range(1, 33):
        for m in range(1, 17):
            b = wsb(n, m, 30, 10000)
            assert (n == 32 or wsb(n + 1, m, 30, 10000) >= b) and (m == 16 or wsb(n, m + 1, 30, 10000) >= b)
    # invalid sizes have no workspace
    assert lib.irs_smooth_values_workspace_bytes(0, 1, 30, 100) == 0
    assert lib.irs_smooth_values_workspace_bytes(2, 1, 1025, 100) == 0
    assert lib.irs_smooth_values_workspace_bytes(2, 1, 30, 0) == 0


def test_geometry_is_a_function_of_T_and_N(lib):
    out = (ctypes.c_longlong * 4)()
    assert lib.irs_smooth_values_geometry(1, 256, out) == 0 and list(out)[:3] == [256, 1, 256]
    assert lib.irs_smooth_values_geometry(1, 257, out) == 0 and list(out)[:3] == [256, 2, 256]
    assert lib.irs_smooth_values_geometry(3, 1000, out) == 0 and list(out)[:3] == [256, 4, 256]
    for T, N in ((30, 10000), (50, 100000), (1024, 1000000), (1, 1)):
        assert lib.irs_smooth_values_geometry(T, N, out) == 0
        block, nblk, chunk = list(out)[:3]
        assert block == 256 and chunk % 256 == 0 and nblk >= 1
        assert (nblk - 1) * chunk < N <= nblk * chunk           # every workgroup has samples, all are covered
        # the workspace holds the partials of this geometry (its size is a bound that is monotone in T and N)
        for n, m in ((2, 1), (32, 16)):
            need = T * nblk * closed_form(n, m) * 8
            assert need <= lib.irs_smooth_values_workspace_bytes(n, m, T, N) <= 4096 * closed_form(n, m) * 8 + 256
    assert lib.irs_smooth_values_geometry(0, 10, out) == INVALID_ARG
    assert lib.irs_smooth_values_geometry(3, 0, out) == INVALID_ARG
    assert lib.irs_smooth_values_geometry(3, 10, None) == INVALID_ARG


def call_accumulate(lib, n=2, m=1, T=3, N=100, dx=ONE, du=ONE, fz=ONE, f0=ONE, sums=ONE, ws=ONE, nbytes=None):
    if nbytes is None:
        nbytes = lib.irs_smooth_values_workspace_bytes(2, 1, 3, 100)
    return lib.irs_smooth_values_accumulate(n, m, T, N, dx, du, fz, f0, sums, ws, nbytes, None)


def call_finalize(lib, n=2, m=1, T=3, N=100, x=ONE, u=ONE, fnom=ONE, sums=ONE, At=ONE, Bt=ONE, ct=ONE, info=ONE):
    return lib.irs_smooth_values_finalize(n, m, T, N, x, u, fnom, sums, At, Bt, ct, info, None)


def call_fused(lib, n=2, m=1, T=3, N=100, x=ONE, u=ONE, dx=ONE, du=ONE, fz=ONE, f0=ONE, fnom=ONE, sums=ONE, At=ONE,
               Bt=ONE, ct=ONE, info=ONE, ws=ONE, nbytes=None):
    if nbytes is None:
        nbytes = lib.irs_smooth_values_workspace_bytes(2, 1, 3, 100)
    return lib.irs_smooth_values(n, m, T, N, x, u, dx, du, fz, f0, fnom, sums, At, Bt, ct, info, ws, nbytes, None)


ENTRIES = [call_accumulate, call_finalize, call_fused]


@pytest.mark.parametrize("call", ENTRIES, ids=["accumulate", "finalize", "fused"])
@pytest.mark.parametrize("bad", [dict(n=0), dict(n=33), dict(m=0), dict(m=17), dict(T=0), dict(T=1025), dict(N=0)],
                         ids=lambda b: "%s=%d" % next(iter(b.items())))
def test_size_errors(lib, call, bad):
    assert call(lib, **bad) == INVALID_ARG
    assert lib.irs_last_error() != b""


@pytest.mark.parametrize("call,names", [
    (call_accumulate, ("dx", "du", "fz", "f0", "sums")),
    (call_finalize, ("x", "u", "fnom", "sums", "At", "Bt", "ct", "info")),
    (call_fused, ("x", "u", "dx", "du", "fz", "f0", "fnom", "sums", "At", "Bt", "ct", "info")),
], ids=["accumulate", "finalize", "fused"])
def test_null_pointer_errors(lib, call, names):
    for name in names:
        assert call(lib, **{name: None}) == INVALID_ARG, name
        assert b"null pointer" in lib.irs_last_error(), name


@pytest.mark.parametrize("call", [call_accumulate, call_fused], ids=["accumulate", "fused"])
def test_sample_alignment_errors(lib, call):
    for name in ("dx", "du", "fz"):
        assert call(lib, **{name: ONE + 4}) == INVALID_ARG, name
        assert b"16-byte aligned" in lib.irs_last_error()


@pytest.mark.parametrize("call", [call_accumulate, call_fused], ids=["accumulate", "fused"])
def test_workspace_errors(lib, call):
    """(finalize takes no workspace.)"""
    need = lib.irs_smooth_values_workspace_bytes(2, 1, 3, 100)
    assert call(lib, ws=None) == WORKSPACE and lib.irs_last_error() != b""
    assert call(lib, nbytes=need - 1) == WORKSPACE and b"workspace" in lib.irs_last_error()
    assert call(lib, nbytes=0) == WORKSPACE
    assert call(lib, ws=ONE + 64) == WORKSPACE and b"256-byte aligned" in lib.irs_last_error()


def test_any_size_rng_samples_errors(lib):
    from irs_mpc_amd._lib import dbl_array
    sx, su = dbl_array([0.1] * 4), dbl_array([0.1])
    for n, m, T, N in ((0, 1, 3, 10), (33, 1, 3, 10), (4, 0, 3, 10), (4, 17, 3, 10), (4, 1, 0, 10), (4, 1, 1025, 10),
                       (4, 1, 3, 0)):
        assert lib.irs_values_rng_samples(n, m, T, N, sx, su, 1, 1, 0, ONE, ONE, None) == INVALID_ARG, (n, m, T, N)
        assert lib.irs_last_error() != b""
    assert lib.irs_values_rng_samples(4, 1, 3, 10, None, su, 1, 1, 0, ONE, ONE, None) == INVALID_ARG
    assert lib.irs_values_rng_samples(4, 1, 3, 10, sx, su, 1, 1, 0, ONE, None, None) == INVALID_ARG
    assert b"null pointer" in lib.irs_last_error()


def test_torch_system_is_exported_and_checks_its_sizes():
    import irs_mpc_amd
    from irs_mpc_amd import all as amd_all
    assert amd_all.TorchDynamicalSystem is irs_mpc_amd.TorchDynamicalSystem
    assert issubclass(irs_mpc_amd.TorchDynamicalSystem, irs_mpc_amd.DynamicalSystem)

    class TooWide(irs_mpc_amd.TorchDynamicalSystem):
        def __init__(self):
            super().__init__()
            self.h, self.dim_x, self.dim_u = 0.1, 33, 1

    with pytest.raises(ValueError, match="dim_x <= 32"):
        TooWide().dm()

    class NoModel(irs_mpc_amd.DynamicalSystem):
        pass

    with pytest.raises(NotImplementedError, match="TorchDynamicalSystem"):
        NoModel().dm()


def test_gpu_accuracy_inputs_are_certified_on_the_cpu():
    """The inputs tests/test_values_pass_gpu.py relies on: the design is well conditioned (cond(Z) about 3 from
    N >= 4 d on), and NumPy in the kernel's form -- statistics in f32, solve in f64 -- stays inside the sample pass's
    stated tolerance of the f64 lstsq statement on exactly these inputs."""
    import numpy as np

    from tests.helpers import values_cases as vc
    tol = dict(rtol=1e-4, atol=2e-5)                 # TOL_AB of tests/test_gpu_parity.py
    for n, m in vc.SIZES:
        for N in vc.sample_counts(n, m):
            assert N >= 4 * (n + m)
            c = vc.make_case(n, m, 3, N)
            Z, _ = vc.design(c)
            assert max(np.linalg.cond(Z[t]) for t in range(3)) < 4.0, (n, m, N)
            for got, ref in zip(vc.f32_gram_f64_solve(c), vc.reference(c)):
                np.testing.assert_allclose(got, ref, **tol)
