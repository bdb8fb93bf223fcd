"""Model-free CEM rollout stages (irs_cem_values_stage, irs_cem_values_stage_drawn), the part that needs no GPU: the
two entries are declared, exported and bound, and every argument error comes back as IRS_ERR_INVALID_ARG with the
entry's name in irs_last_error() -- on a machine without a GPU, so the decision precedes any HIP call."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
NEW = ("irs_cem_values_stage", "irs_cem_values_stage_drawn")
ONE = 256       # any non-null address: validation happens before anything is dereferenced
POINTERS = {"irs_cem_values_stage": ("x", "u_cand", "Q", "R", "xd_trj", "u_t", "costs"),
            "irs_cem_values_stage_drawn": ("x", "u_mean", "std", "Q", "R", "xd_trj", "u_t", "costs")}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from irs_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.load()


def test_new_symbols_are_declared_exported_and_bound(lib):
    from irs_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "irs_hip.h")).read()
    for s in NEW:
        assert s + "(" in header, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    assert lib.irs_abi_version() == 1


def stage(lib, entry, n=4, m=2, T=5, B=100, t=0, null=None):
    p = {k: ONE for k in POINTERS[entry]}
    if null is not None:
        p[null] = None
    if entry == "irs_cem_values_stage":
        return lib.irs_cem_values_stage(n, m, T, B, t, p["x"], p["u_cand"], p["Q"], p["R"], p["xd_trj"], p["u_t"],
                                        p["costs"], None)
    return lib.irs_cem_values_stage_drawn(n, m, T, B, t, p["x"], p["u_mean"], p["std"], 7, 1, 0, p["Q"], p["R"],
                                          p["xd_trj"], p["u_t"], p["costs"], None)


@pytest.mark.parametrize("entry", NEW)
def test_stage_argument_errors_without_gpu(lib, entry):
    def refused(**kw):
        rc = stage(lib, entry, **kw)
        assert rc == INVALID, (kw, rc)
        assert entry.encode() + b":" in lib.irs_last_error(), (kw, lib.irs_last_error())

    for kw in (dict(n=0), dict(n=-1), dict(n=33), dict(m=0), dict(m=-3), dict(m=17),
               dict(T=0), dict(T=-2), dict(B=0), dict(B=-1),
               dict(t=-1), dict(t=6), dict(T=1, t=2)):
        refused(**kw)
    for name in POINTERS[entry]:
        refused(null=name)                  # t = 0 < T: u_t is needed too
    # at the terminal stage u_t is ignored; every other pointer is still needed
    for name in POINTERS[entry]:
        if name != "u_t":
            refused(t=5, null=name)
