"""Calls into the fifteen sample-pass entries of the C ABI (csrc/smooth_api.hip) that must be refused BEFORE any
launch: every argument check, in every entry, and -- where two checks would fire -- which of them wins.  Pointers are
fake non-null addresses: a refused call dereferences nothing, and no GPU is opened.

cases() is the table, run(lib) its (return code, irs_last_error text) per (entry, case); size_cases() / sizes(lib) are
the four size queries on a few dozen (model, mode, T, N, B).  The results of the library as it stood while these
entries still marshalled and checked by hand in csrc/smooth.hip are tests/golden/smooth_entry_errors.json;
tests/test_smooth_entries_cpu.py holds every later library to them.
`python -m tests.helpers.smooth_entry_cases OUT.json` records both tables from the library in the tree (or IRS_HIP_LIB).

No recorded number may depend on the machine.  The one that could is the workgroup count of the uniform-geometry family
(the CU count; IRS_MODEL_PLANAR_HAND_EXACT in the u-only modes): it enters irs_smooth_workspace_bytes.  Every shape of
that family here has N <= 448 -- at most seven 64-sample blocks, which one workgroup's eight waves take whatever the CU
count -- so its count is 1 everywhere."""
import ctypes
import json
import os
import sys

from irs_mpc_amd import _lib

PEND, QUAD, HAND, HAND_EXACT = _lib.MODEL_PENDULUM, _lib.MODEL_QUADROTOR, _lib.MODEL_PLANAR_HAND, _lib.MODEL_PLANAR_HAND_EXACT
AB, FIRST, ZB = _lib.SMOOTH_ZERO_ORDER_AB, _lib.SMOOTH_FIRST_ORDER, _lib.SMOOTH_ZERO_ORDER_B
UNKNOWN = 99
PTR, ODD = 0x10000, 0x10008        # a 16-byte aligned address, one that is not
WS, WS_OFF = 0x20000, 0x20010      # a 256-byte aligned workspace address, one that is only 16-byte aligned
BIG = 1 << 30
GENERAL = {"IRS_UG": "0"}          # the environment of a call that must take the general kernel

HEAD = ["model", "params", "n_params", "mode", "T", "N", "x_trj", "u_trj"]
OUTS = ["At", "Bt", "ct", "info"]
TAIL = ["workspace", "workspace_bytes", "stream"]
# entry -> its parameters in order (include/irs_hip.h)
ENTRIES = {
    "irs_smooth": HEAD + ["dx", "du", "sums"] + OUTS + TAIL,
    "irs_smooth_rng": HEAD + ["std_x", "std_u", "seed", "iter", "sums"] + OUTS + TAIL,
    "irs_smooth_accumulate": HEAD + ["dx", "du", "sums"] + TAIL,
    "irs_smooth_accumulate_rng": HEAD + ["std_x", "std_u", "seed", "iter", "sample_offset", "sums"] + TAIL,
    "irs_smooth_run": ["call", "stream"],
    "irs_smooth_rng_batch": HEAD[:6] + ["B", "x_trj", "x_stride", "u_trj", "u_stride", "std_u_dev", "seed_dev", "iter",
                                        "sums"] + OUTS + TAIL,
    "irs_smooth_rng_general_batch": HEAD[:6] + ["B", "x_trj", "x_stride", "u_trj", "u_stride", "std_x_dev", "std_u_dev",
                                                "seed_dev", "iter", "sums"] + OUTS + TAIL,
    "irs_smooth_finalize": HEAD[:5] + ["n_total", "x_trj", "u_trj", "sums"] + OUTS + ["stream"],
    "irs_smooth_finalize_ws": HEAD[:5] + ["n_total", "x_trj", "u_trj", "sums"] + OUTS + TAIL,
    "irs_rng_samples": ["n", "m", "T", "N", "std_x", "std_u", "seed", "iter", "sample_offset", "dx", "du", "stream"],
    "irs_exact_linearize": ["model", "params", "n_params", "T", "x_trj", "u_trj", "At", "Bt", "ct", "stream"],
    "irs_workspace_init": TAIL,
    "irs_smooth_batch_workspace_init": TAIL,
    "irs_smooth_general_batch_workspace_init": TAIL,
    "irs_smooth_geometry": ["model", "mode", "T", "N", "rng", "geometry_out"],
}
SINGLE = ("irs_smooth", "irs_smooth_rng", "irs_smooth_accumulate", "irs_smooth_accumulate_rng", "irs_smooth_run")

# what a call that would run looks like (never made): every case below overrides at least one of these so that it
# is refused.  "model" stands for (model, params, n_params); std_x / std_u True = an array, None = a null pointer
BASE = dict(model=PEND, mode=AB, T=10, N=100, B=3, n=2, m=1, rng=0, x_trj=PTR, u_trj=PTR, dx=PTR, du=PTR, std_x=True,
            std_u=True, std_x_dev=PTR, std_u_dev=PTR, seed_dev=PTR, seed=7, iter=1, sample_offset=0, sums=PTR, At=PTR, Bt=PTR, ct=PTR,
            info=PTR, n_total=100, workspace=WS, workspace_bytes=BIG, stream=None, x_stride=BIG, u_stride=BIG,
            use_rng=0, fuse=True, geometry_out=True, env={})
U_ONLY = dict(model=HAND, mode=ZB)             # a mode that never reads dx / std_x
SERVED = dict(model=HAND_EXACT, mode=ZB, T=3, N=64)     # what the batch entry serves; one workgroup on any machine
SERVED_GENERAL = dict(model=PEND, mode=AB, T=3, N=64)   # what the general batch entry serves (n = 2, m = 1)
GENERAL_SLICE = 5120      # that shape's workspace slice: round256(irs_smooth_workspace_bytes) (sizes() records it, B = 1)


def _single_cases(entry):
    rng = entry.endswith("_rng")
    fused = entry in ("irs_smooth", "irs_smooth_rng")
    by_struct = entry == "irs_smooth_run"
    out = [("T_zero", dict(T=0)), ("N_zero", dict(N=0)), ("N_negative", dict(N=-5)),
           ("null_x_trj", dict(x_trj=None)), ("null_u_trj", dict(u_trj=None)), ("null_sums", dict(sums=None)),
           ("null_workspace", dict(workspace=None)), ("mode_three", dict(mode=3)), ("mode_negative", dict(mode=-1)),
           ("unknown_model", dict(model=UNKNOWN)), ("unknown_model_u_only", dict(model=UNKNOWN, mode=ZB)),
           ("unknown_model_first_order", dict(model=UNKNOWN, mode=FIRST)),
           ("param_count", dict(n_params=3)),
           ("T_beyond_counters", dict(T=1025)), ("T_at_counters_small_workspace", dict(T=1024, workspace_bytes=8)),
           ("small_workspace", dict(workspace_bytes=8)), ("small_workspace_contact", dict(workspace_bytes=8, **U_ONLY)),
           ("small_workspace_quadrotor", dict(model=QUAD, T=50, N=10000, workspace_bytes=4096)),
           ("small_workspace_uniform_geometry", dict(workspace_bytes=8, **SERVED)),
           ("small_workspace_general_kernel", dict(workspace_bytes=8, env=GENERAL, **SERVED)),
           # which of two faults is reported
           ("T_zero_and_null_x_trj", dict(T=0, x_trj=None)), ("null_x_trj_and_mode_three", dict(x_trj=None, mode=3)),
           ("mode_three_and_T_beyond_counters", dict(mode=3, T=1025)),
           ("T_beyond_counters_and_unknown_model", dict(T=1025, model=UNKNOWN)),
           ("T_beyond_counters_and_param_count", dict(T=1025, n_params=3)),
           ("param_count_and_small_workspace", dict(n_params=3, workspace_bytes=8)),
           ("unknown_model_and_small_workspace", dict(model=UNKNOWN, workspace_bytes=8))]
    if not by_struct:
        out += [("null_params", dict(params=None)), ("null_params_and_small_workspace", dict(params=None, workspace_bytes=8))]
    samples, drawn = [], []
    if not rng:
        samples = [("null_du", dict(du=None)), ("null_dx", dict(dx=None)),
                   ("null_dx_analytic_first_order", dict(dx=None, mode=FIRST)),
                   # allowed in the u-only modes: the call gets past that check, and the next fault is reported
                   ("null_dx_u_only_then_T_zero", dict(dx=None, T=0, **U_ONLY)),
                   ("null_dx_contact_first_order_then_null_sums", dict(dx=None, model=HAND, mode=FIRST, sums=None)),
                   ("null_dx_unknown_model_then_mode_three", dict(dx=None, model=UNKNOWN, mode=3)),
                   ("misaligned_dx", dict(dx=ODD)), ("misaligned_du", dict(du=ODD)),
                   ("misaligned_du_u_only_null_dx", dict(dx=None, du=ODD, **U_ONLY)),
                   ("null_du_and_T_zero", dict(du=None, T=0)), ("null_du_and_null_dx", dict(du=None, dx=None)),
                   ("null_dx_and_misaligned_du", dict(dx=None, du=ODD)),
                   ("misaligned_dx_and_null_sums", dict(dx=ODD, sums=None)),
                   ("misaligned_dx_and_unknown_model", dict(dx=ODD, model=UNKNOWN))]
    if rng:
        drawn = [("null_std_u", dict(std_u=None)), ("null_std_x", dict(std_x=None)),
                 ("null_std_x_analytic_first_order", dict(std_x=None, mode=FIRST)),
                 ("null_std_x_u_only_then_T_zero", dict(std_x=None, T=0, **U_ONLY)),
                 ("null_std_x_contact_first_order_then_null_sums", dict(std_x=None, model=HAND, mode=FIRST, sums=None)),
                 ("null_std_x_unknown_model", dict(std_x=None, model=UNKNOWN)),
                 ("null_std_u_and_null_std_x", dict(std_u=None, std_x=None)),
                 ("null_std_u_and_T_zero", dict(std_u=None, T=0)),
                 ("null_std_u_and_unknown_model", dict(std_u=None, model=UNKNOWN))]
    if by_struct:
        # both sample sources of the struct, and both of its forms (At set: fused; At null: accumulate only)
        out = [(name + "_drawn", dict(over, use_rng=1)) for name, over in out] + out + samples
        out += [("null_call", dict(call=None)),
                ("drawn_ignores_null_du_then_T_zero", dict(use_rng=1, du=None, T=0)),
                ("supplied_u_only_null_dx_then_small_workspace", dict(dx=None, workspace_bytes=8, **U_ONLY)),
                ("n_total_zero", dict(n_total=0)), ("n_total_negative", dict(n_total=-1)),
                ("n_total_zero_drawn", dict(n_total=0, use_rng=1)),
                ("accumulate_only_T_zero", dict(fuse=False, T=0)),
                ("accumulate_only_small_workspace", dict(fuse=False, workspace_bytes=8)),
                ("accumulate_only_null_sums_drawn", dict(fuse=False, use_rng=1, sums=None))]
        fused = True
    out += samples + drawn if not by_struct else []
    if fused:
        # the outputs are looked at last: behind the workspace and the planner
        out += [("null_Bt", dict(Bt=None)), ("null_ct", dict(ct=None)), ("null_info", dict(info=None)),
                ("null_Bt_uniform_geometry", dict(Bt=None, **SERVED)),
                ("null_info_general_kernel", dict(info=None, env=GENERAL, **SERVED)),
                ("null_info_and_small_workspace", dict(info=None, workspace_bytes=8)),
                ("null_ct_and_T_zero", dict(ct=None, T=0)), ("null_Bt_and_unknown_model", dict(Bt=None, model=UNKNOWN))]
        if not by_struct:      # (by struct a null At asks for the accumulate-only form: that call would run)
            out += [("null_At", dict(At=None)), ("no_outputs", dict(At=None, Bt=None, ct=None, info=None))]
    return out


def _batch_cases():
    s = SERVED
    nulls = [("null_" + k, dict(s, **{k: None})) for k in ("x_trj", "u_trj", "std_u_dev", "seed_dev", "sums", "At", "Bt",
                                                            "ct", "info")]
    return nulls + [
        ("B_zero", dict(s, B=0)), ("T_zero", dict(s, T=0)), ("N_zero", dict(s, N=0)),
        ("T_beyond_counters", dict(s, T=1025)), ("rows_beyond_grid", dict(s, B=100, T=700)),
        ("rows_at_grid_small_workspace", dict(s, B=21845, T=3, workspace_bytes=8)),
        ("mode_three", dict(s, mode=3)), ("mode_negative", dict(s, mode=-1)),
        ("unknown_model", dict(s, model=UNKNOWN)), ("analytic_model", dict(s, model=PEND)),
        ("swept_contact_model", dict(s, model=HAND)), ("zero_order_ab", dict(s, mode=AB)),
        ("first_order_small_workspace", dict(s, mode=FIRST, workspace_bytes=8)),
        ("general_kernel", dict(s, env=GENERAL)), ("general_kernel_first_order", dict(s, mode=FIRST, env=GENERAL)),
        ("param_count", dict(s, n_params=3)), ("null_params", dict(s, params=None)),
        ("short_x_stride", dict(s, x_stride=20)), ("short_u_stride", dict(s, u_stride=11)),
        ("x_stride_exact_small_workspace", dict(s, x_stride=21, u_stride=12, workspace_bytes=8)),
        ("null_workspace", dict(s, workspace=None)), ("small_workspace", dict(s, workspace_bytes=8)),
        ("small_workspace_one_slice", dict(s, B=1, workspace_bytes=4096)),
        ("misaligned_workspace", dict(s, workspace=WS_OFF)),
        # which of two faults is reported
        ("B_zero_and_null_sums", dict(s, B=0, sums=None)),
        ("T_beyond_counters_and_rows_beyond_grid", dict(s, T=1025, B=100)),
        ("rows_beyond_grid_and_null_x_trj", dict(s, B=100, T=700, x_trj=None)),
        ("null_info_and_mode_three", dict(s, info=None, mode=3)),
        ("mode_three_and_unknown_model", dict(s, mode=3, model=UNKNOWN)),
        ("analytic_model_and_param_count", dict(s, model=PEND, n_params=3)),
        ("general_kernel_and_null_params", dict(s, params=None, env=GENERAL)),
        ("param_count_and_short_x_stride", dict(s, n_params=3, x_stride=20)),
        ("short_u_stride_and_null_workspace", dict(s, u_stride=11, workspace=None)),
        ("small_and_misaligned_workspace", dict(s, workspace=WS_OFF, workspace_bytes=8)),
        ("null_and_small_workspace", dict(s, workspace=None, workspace_bytes=8))]


def _general_batch_cases():
    s = SERVED_GENERAL
    nulls = [("null_" + k, dict(s, **{k: None})) for k in ("x_trj", "u_trj", "std_x_dev", "std_u_dev", "seed_dev", "sums",
                                                            "At", "Bt", "ct", "info")]
    return nulls + [
        ("B_zero", dict(s, B=0)), ("T_zero", dict(s, T=0)), ("N_zero", dict(s, N=0)),
        ("T_beyond_counters", dict(s, T=1025)), ("rows_beyond_grid", dict(s, B=100, T=700)),
        ("rows_at_grid_small_workspace", dict(s, B=21845, T=3, workspace_bytes=8)),
        ("mode_three", dict(s, mode=3)), ("mode_negative", dict(s, mode=-1)),
        ("unknown_model", dict(s, model=UNKNOWN)), ("swept_contact_model", dict(s, model=HAND)),
        ("swept_contact_model_first_order", dict(s, model=HAND, mode=FIRST)),
        ("planar_hand_exact", dict(s, model=HAND_EXACT)), ("planar_hand_exact_u_only", dict(s, model=HAND_EXACT, mode=ZB)),
        ("planar_hand_exact_general_kernel", dict(s, model=HAND_EXACT, mode=ZB, env=GENERAL)),
        ("zero_order_b", dict(s, mode=ZB)), ("zero_order_b_quadrotor", dict(s, model=QUAD, mode=ZB)),
        ("first_order_small_workspace", dict(s, mode=FIRST, workspace_bytes=8)),
        ("quadrotor_small_workspace", dict(s, model=QUAD, workspace_bytes=8)),
        ("param_count", dict(s, n_params=3)), ("null_params", dict(s, params=None)),
        ("short_x_stride", dict(s, x_stride=5)), ("short_u_stride", dict(s, u_stride=2)),
        ("x_stride_exact_small_workspace", dict(s, x_stride=6, u_stride=3, workspace_bytes=8)),
        ("null_workspace", dict(s, workspace=None)), ("small_workspace", dict(s, workspace_bytes=8)),
        ("small_workspace_one_slice", dict(s, B=1, workspace_bytes=4096)),
        ("workspace_one_slice_short", dict(s, workspace_bytes=2 * GENERAL_SLICE)),
        ("workspace_one_byte_short", dict(s, workspace_bytes=3 * GENERAL_SLICE - 1)),
        ("misaligned_workspace", dict(s, workspace=WS_OFF)),
        # which of two faults is reported
        ("B_zero_and_T_beyond_counters", dict(s, B=0, T=1025)),
        ("B_zero_and_null_sums", dict(s, B=0, sums=None)),
        ("T_beyond_counters_and_rows_beyond_grid", dict(s, T=1025, B=100)),
        ("rows_beyond_grid_and_null_std_x_dev", dict(s, B=100, T=700, std_x_dev=None)),
        ("null_info_and_mode_three", dict(s, info=None, mode=3)),
        ("mode_three_and_unknown_model", dict(s, mode=3, model=UNKNOWN)),
        ("swept_contact_model_and_param_count", dict(s, model=HAND, n_params=3)),
        ("zero_order_b_and_null_params", dict(s, mode=ZB, params=None)),
        ("param_count_and_short_x_stride", dict(s, n_params=3, x_stride=5)),
        ("short_u_stride_and_null_workspace", dict(s, u_stride=2, workspace=None)),
        ("small_and_misaligned_workspace", dict(s, workspace=WS_OFF, workspace_bytes=8)),
        ("null_and_small_workspace", dict(s, workspace=None, workspace_bytes=8))]


def _finalize_cases(entry):
    out = [("T_zero", dict(T=0)), ("n_total_zero", dict(n_total=0)), ("n_total_negative", dict(n_total=-3)),
           ("mode_three", dict(mode=3)), ("mode_negative", dict(mode=-1)), ("unknown_model", dict(model=UNKNOWN)),
           ("param_count", dict(n_params=3)), ("null_params", dict(params=None)),
           ("T_zero_and_null_sums", dict(T=0, sums=None)), ("null_At_and_mode_three", dict(At=None, mode=3)),
           ("mode_three_and_unknown_model", dict(mode=3, model=UNKNOWN)),
           ("unknown_model_contact_mode", dict(model=UNKNOWN, mode=ZB))]
    out += [("null_" + k, {k: None}) for k in ("x_trj", "u_trj", "sums", "At", "Bt", "ct", "info")]
    if entry.endswith("_ws"):
        # a workspace that is given must hold the counters and T rows of nominal steps (4096 + 256 T bytes)
        out += [("small_workspace", dict(workspace_bytes=8)), ("workspace_one_byte_short", dict(workspace_bytes=4096 + 2560 - 1)),
                ("workspace_long_horizon", dict(model=HAND, mode=ZB, T=50, workspace_bytes=4096 + 12799)),
                ("T_zero_and_small_workspace", dict(T=0, workspace_bytes=8)),
                ("small_workspace_and_null_sums", dict(workspace_bytes=8, sums=None)),
                ("small_workspace_and_unknown_model", dict(workspace_bytes=8, model=UNKNOWN)),
                ("no_workspace_null_sums", dict(workspace=None, workspace_bytes=0, sums=None))]
    return out


def entry_cases(entry):
    """(case name, overrides) of one entry."""
    if entry in SINGLE:
        return _single_cases(entry)
    if entry == "irs_smooth_rng_batch":
        return _batch_cases()
    if entry == "irs_smooth_rng_general_batch":
        return _general_batch_cases()
    if "finalize" in entry:
        return _finalize_cases(entry)
    if entry == "irs_rng_samples":
        return [("T_zero", dict(T=0)), ("N_zero", dict(N=0)), ("null_dx", dict(dx=None)), ("null_du", dict(du=None)),
                ("null_std_x", dict(std_x=None)), ("null_std_u", dict(std_u=None)),
                ("unregistered_sizes", dict(n=3, m=3)), ("unregistered_swapped_sizes", dict(n=1, m=2)),
                ("unregistered_state_only", dict(n=7, m=2)), ("unregistered_sizes_and_T_zero", dict(n=3, m=3, T=0)),
                ("unregistered_sizes_and_null_std_x", dict(n=3, m=3, std_x=None))]
    if entry == "irs_exact_linearize":
        return [("T_zero", dict(T=0)), ("unknown_model", dict(model=UNKNOWN)), ("param_count", dict(n_params=3)),
                ("null_params", dict(params=None)), ("T_zero_and_unknown_model", dict(T=0, model=UNKNOWN)),
                ("null_ct_and_param_count", dict(ct=None, n_params=3))] \
            + [("null_" + k, {k: None}) for k in ("x_trj", "u_trj", "At", "Bt", "ct")]
    if entry == "irs_workspace_init":
        return [("null_workspace", dict(workspace=None)), ("no_bytes", dict(workspace_bytes=0)),
                ("one_byte_short", dict(workspace_bytes=4095)), ("null_and_short", dict(workspace=None, workspace_bytes=8))]
    if entry in ("irs_smooth_batch_workspace_init", "irs_smooth_general_batch_workspace_init"):
        return [("null_workspace", dict(workspace=None)), ("no_bytes", dict(workspace_bytes=0)),
                ("null_and_no_bytes", dict(workspace=None, workspace_bytes=0))]
    assert entry == "irs_smooth_geometry"
    return [("T_zero", dict(T=0)), ("N_zero", dict(N=0)), ("mode_three", dict(mode=3)), ("mode_negative", dict(mode=-1)),
            ("unknown_model", dict(model=UNKNOWN)), ("unknown_model_drawn", dict(model=UNKNOWN, rng=1)),
            ("null_out", dict(geometry_out=None)), ("null_out_and_T_zero", dict(geometry_out=None, T=0)),
            ("T_zero_and_mode_three", dict(T=0, mode=3)), ("mode_three_and_unknown_model", dict(mode=3, model=UNKNOWN)),
            ("N_zero_general_kernel", dict(SERVED, N=0, env=GENERAL))]


def cases():
    """[(entry, case, overrides)], every entry's cases in a fixed order."""
    return [(entry, name, over) for entry in ENTRIES for name, over in entry_cases(entry)]


def _n_params(lib, model):
    n, m, npar = _lib.c_int(), _lib.c_int(), _lib.c_int()
    return npar.value if lib.irs_model_info(model, n, m, npar) == 0 else 1


class _environment:
    """The tuning variables of one call (read per call by the library), put back afterwards."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.before = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _struct(v, npar):
    c = _lib.SmoothCall()
    c.model, c.n_params, c.mode, c.T, c.N = v["model"], v["n_params"], v["mode"], v["T"], v["N"]
    for i in range(min(npar, 12)):
        c.params[i] = 0.1
    for k in ("x_trj", "u_trj", "dx", "du", "sums", "workspace"):
        setattr(c, k, v[k])
    for k in OUTS:
        setattr(c, k, v[k] if v["fuse"] else None)
    c.use_rng, c.iter, c.seed, c.sample_offset = v["use_rng"], v["iter"], v["seed"], v["sample_offset"]
    c.n_total, c.workspace_bytes = v["n_total"], v["workspace_bytes"]
    for i in range(32):
        c.std_x[i] = 0.1
    for i in range(16):
        c.std_u[i] = 0.1
    return c


def call(lib, entry, over):
    """One call of the table: (return code, irs_last_error text)."""
    v = dict(BASE)
    v.update(over)
    npar = _n_params(lib, v["model"])
    v.setdefault("n_params", npar)
    v.setdefault("params", _lib.dbl_array([0.1] * npar))
    for k in ("std_x", "std_u"):
        v[k] = _lib.dbl_array([0.1] * 32) if v[k] else None
    out = (ctypes.c_int * 8)()
    v["geometry_out"] = out if v["geometry_out"] else None
    if entry == "irs_smooth_run" and "call" not in v:
        c = _struct(v, npar)
        v["call"] = ctypes.byref(c)
    with _environment(v["env"]):
        rc = getattr(lib, entry)(*[v[name] for name in ENTRIES[entry]])
        return rc, lib.irs_last_error().decode("utf-8")


def run(lib):
    """{"<entry>/<case>": [return code, error text]} of the whole table."""
    return {"%s/%s" % (entry, name): list(call(lib, entry, over)) for entry, name, over in cases()}


def size_cases():
    """[(model, mode, T, N, B, environment)] of the size queries: served and unserved models and modes, sizes with one
    and with several workgroups per time step, and arguments that make a query answer 0 or an error code."""
    out = []
    for model, mode in [(PEND, AB), (PEND, FIRST), (PEND, ZB), (QUAD, AB), (QUAD, FIRST), (_lib.MODEL_BICYCLE, AB),
                        (_lib.MODEL_THREE_CART, ZB), (HAND, AB), (HAND, FIRST), (HAND, ZB), (_lib.MODEL_BOX_PIVOT, ZB),
                        (_lib.MODEL_BOX_ON_BOX, AB), (_lib.MODEL_BOX_PUSH, FIRST), (_lib.MODEL_BOX_PIVOT_EXACT, ZB),
                        (_lib.MODEL_BOX_PUSH_EXACT, FIRST)]:
        out += [(model, mode, 3, 1000, 3, {}), (model, mode, 50, 10000, 2, {}), (model, mode, 1024, 100000, 1, {})]
    for mode in (FIRST, ZB):
        out += [(HAND_EXACT, mode, T, N, B, env) for T, N, B in ((1, 1, 1), (3, 64, 3), (50, 448, 7), (1024, 300, 2))
                for env in ({}, GENERAL)]
        out += [(HAND_EXACT, mode, 50, 10000, 4, GENERAL)]
    out += [(HAND_EXACT, AB, 50, 10000, 3, {}), (UNKNOWN, AB, 3, 100, 1, {}), (UNKNOWN, ZB, 3, 100, 1, GENERAL),
            (PEND, 3, 3, 100, 1, {}), (HAND_EXACT, -1, 3, 100, 1, {}), (PEND, AB, 0, 100, 1, {}), (PEND, AB, 3, 0, 1, {}),
            (HAND_EXACT, ZB, 3, 64, 0, {}), (HAND_EXACT, ZB, 0, 64, 3, {}), (HAND_EXACT, ZB, 3, -1, 3, {}),
            (HAND_EXACT, FIRST, 3, 64, -2, {})]
    # what the general batch entry serves, and does not
    out += [(PEND, FIRST, 3, 64, 1, {}), (PEND, AB, 3, 64, 1, {}), (QUAD, FIRST, 50, 448, 7, {}), (PEND, AB, 3, 64, 0, {}),
            (QUAD, FIRST, 3, 64, -2, {}), (PEND, ZB, 3, 64, 3, {})]
    return out


def size_key(case):
    model, mode, T, N, B, env = case
    return "model%d/mode%d/T%d/N%d/B%d%s" % (model, mode, T, N, B, "/general" if env else "")


def sizes(lib):
    """{key: [irs_sums_len, irs_smooth_workspace_bytes, irs_smooth_batch_workspace_bytes,
    irs_smooth_general_batch_workspace_bytes]}."""
    out = {}
    for case in size_cases():
        model, mode, T, N, B, env = case
        with _environment(env):
            out[size_key(case)] = [lib.irs_sums_len(model, mode), lib.irs_smooth_workspace_bytes(model, mode, T, N),
                                   lib.irs_smooth_batch_workspace_bytes(model, mode, T, N, B),
                                   lib.irs_smooth_general_batch_workspace_bytes(model, mode, T, N, B)]
    return out


if __name__ == "__main__":
    lib = _lib.load()
    with open(sys.argv[1], "w") as f:
        json.dump({"refusals": run(lib), "sizes": sizes(lib)}, f, indent=0, sort_keys=True)
        f.write("\n")
