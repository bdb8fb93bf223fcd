"""Calls into the fourteen bounded-ADMM entries of the C ABI (csrc/boxqp_api.hip) that must be refused BEFORE any
launch: every argument check, in every entry, and -- where two checks would fire -- which of them wins.  Pointers are
fake non-null addresses: a refused call dereferences nothing, and no GPU is opened.

cases() is the table, run(lib) its (return code, irs_last_error text) per (entry, case).  The results of the library
as it stood before the entries moved to their own file are tests/golden/box_entry_errors.json;
tests/test_box_entries_cpu.py holds every later library to them.  `python -m tests.helpers.box_entry_cases OUT.json`
records the table from the library in the tree (or IRS_HIP_LIB)."""
import ctypes
import json
import sys

from irs_mpc_amd import _lib

QUAD, BICYCLE, HAND = _lib.MODEL_QUADROTOR, _lib.MODEL_BICYCLE, _lib.MODEL_PLANAR_HAND
UNKNOWN = 99
ONE = 8                 # any non-null address
WS, OFF = 256, 264      # a 256-byte aligned workspace address, a misaligned one
BIG = 1 << 30

PROBLEM = ["At", "Bt", "ct", "Q", "Qd", "R"]
HEAD = ["model", "params", "n_params", "T"] + PROBLEM
DESCENT = HEAD + ["alpha_R", "xd_trj", "x0", "xlo", "xhi", "ulo", "uhi"]
SOLVE = HEAD + ["alpha_R", "xd_trj", "x0", "position_controlled", "x_lo", "x_hi", "u_lo", "u_hi", "du_lo", "du_hi"]
QUASI = HEAD + ["xd_trj", "x0", "x_lo", "x_hi", "u_lo", "u_hi", "du_lo", "du_hi", "solver"]
SCALARS = ["rho", "relax", "max_iter", "eps"]
WSP = ["workspace", "workspace_bytes"]
LAZY = ["enforced_io", "lazy_out"]

# entry -> its parameters in order (include/irs_hip.h)
ENTRIES = {
    "irs_tvlqr_box_descent": DESCENT + SCALARS + ["x_new", "u_new", "info", "stream"],
    "irs_tvlqr_box_descent_if": DESCENT + SCALARS + ["x_new", "u_new", "cost", "info", "run_flag", "stream"],
    "irs_tvlqr_box_descent_wsx": DESCENT + SCALARS + ["x_new", "u_new", "info"] + WSP + ["stream"],
    "irs_tvlqr_box_descent_set": DESCENT + ["settings", "x_new", "u_new", "info", "adapt_out"] + WSP + ["stream"],
    "irs_tvlqr_box_descent_lazy": DESCENT + ["settings", "x_new", "u_new", "info", "adapt_out"] + WSP + LAZY + ["stream"],
    "irs_tvlqr_box_solve": SOLVE + SCALARS + ["x_new", "u_new", "info", "stream"],
    "irs_tvlqr_box_solve_wsx": SOLVE + SCALARS + ["x_new", "u_new", "info"] + WSP + ["stream"],
    "irs_tvlqr_box_solve_set": SOLVE + ["settings", "x_new", "u_new", "info", "adapt_out"] + WSP + ["stream"],
    "irs_tvlqr_box_solve_lazy": SOLVE + ["settings", "x_new", "u_new", "info", "adapt_out"] + WSP + LAZY + ["stream"],
    "irs_quasistatic_box_descent": QUASI + SCALARS + ["x_new", "u_new", "cost", "info", "stream"],
    "irs_quasistatic_box_descent_ws": QUASI + SCALARS + ["x_new", "u_new", "cost", "info", "act_io", "stream"],
    "irs_quasistatic_box_descent_wsx": QUASI + SCALARS + ["x_new", "u_new", "cost", "info", "act_io"] + WSP + ["stream"],
    "irs_quasistatic_box_descent_set": QUASI + ["settings", "x_new", "u_new", "cost", "info", "adapt_out"] + WSP + ["stream"],
    "irs_quasistatic_box_descent_lazy": QUASI + ["settings", "x_new", "u_new", "cost", "info", "adapt_out"] + WSP + LAZY
                                        + ["stream"],
}

# what a call that would run looks like (never made): every case below overrides at least one of these so that it
# is refused.  "model" stands for (model, params, n_params) and "settings" is a dict of admm_settings keywords
BASE = dict(T=10, alpha_R=0.5, position_controlled=1, solver=1, rho=10.0, relax=1.6, max_iter=100, eps=1e-8,
            settings={}, workspace=None, workspace_bytes=0, stream=None, cost=ONE, run_flag=None, act_io=None,
            adapt_out=None, enforced_io=None, lazy_out=None, x_lo=None, x_hi=None, du_lo=None, du_hi=None)


def _family(entry):
    return "descent" if "tvlqr_box_descent" in entry else "solve" if "solve" in entry else "quasi"


def entry_cases(entry):
    """(case name, overrides) of one entry."""
    names, fam = ENTRIES[entry], _family(entry)
    has_ws, by_settings = "workspace" in names, "settings" in names
    bad = BICYCLE                                    # a model without a position-controlled form
    out = [("T_zero", dict(T=0)), ("null_At", dict(At=None)), ("null_x0", dict(x0=None)), ("null_R", dict(R=None)),
           ("null_x_out", dict(x_new=None)), ("null_u_out", dict(u_new=None)), ("null_info", dict(info=None)),
           ("unknown_model", dict(model=UNKNOWN)), ("param_count", dict(n_params=3)), ("null_params", dict(params=None))]

    # the ADMM settings, positional or in the struct; a null pointer beside bad settings: the pointer is named
    def st(**kw):
        return dict(settings=kw) if by_settings else kw
    out += [("rho_zero", st(rho=0.0)), ("relax_two", st(relax=2.0)), ("relax_zero", st(relax=0.0)),
            ("max_iter_zero", st(max_iter=0)), ("eps_zero", st(eps=0.0)),
            ("null_At_and_rho_zero", dict(At=None, **st(rho=0.0))),
            ("rho_zero_and_unknown_model", dict(model=UNKNOWN, **st(rho=0.0)))]
    if by_settings:
        out += [("null_settings", dict(settings=None)),
                ("check_every_zero", st(adaptive=True, check_every=0)), ("trigger_one", st(adaptive=True, trigger=1.0)),
                ("max_refactor_negative", st(adaptive=True, max_refactor=-1)),
                ("rho_zero_and_check_every_zero", st(rho=0.0, adaptive=True, check_every=0)),
                ("null_settings_and_unknown_model", dict(settings=None, model=UNKNOWN))]

    if fam == "descent":
        # all four bound pointers are required; past the horizon limits on the quadrotor (on chip: T <= 50, HBM: 357)
        out += [("null_xlo", dict(xlo=None)), ("null_uhi", dict(uhi=None)), ("null_x_pair", dict(xlo=None, xhi=None)),
                ("beyond_lds_no_workspace", dict(model=QUAD, T=51))]
        if has_ws:
            out += [("beyond_limit_with_workspace", dict(model=QUAD, T=358, workspace=WS, workspace_bytes=BIG)),
                    ("beyond_limit_small_workspace", dict(model=QUAD, T=358, workspace=WS, workspace_bytes=8))]
    else:
        out += [("one_sided_x", dict(x_lo=ONE)), ("one_sided_u", dict(u_hi=None)), ("one_sided_du", dict(du_hi=ONE)),
                ("null_At_and_one_sided_u", dict(At=None, u_hi=None)),
                ("one_sided_u_and_rho_zero", dict(u_hi=None, **st(rho=0.0))),
                ("not_position_controlled_model", dict(model=bad)),
                ("beyond_lds_no_workspace", dict(T=57))]
        if by_settings:
            out += [("one_sided_u_and_null_settings", dict(u_hi=None, settings=None))]
        if has_ws:
            out += [("beyond_limit_with_workspace", dict(T=384, workspace=WS, workspace_bytes=BIG))]
    if fam == "solve":
        out += [("du_bounds_plain_form", dict(position_controlled=0, du_lo=ONE, du_hi=ONE)),
                ("one_sided_u_and_du_bounds_plain_form", dict(position_controlled=0, du_lo=ONE, du_hi=ONE, u_hi=None)),
                ("du_bounds_plain_form_and_rho_zero", dict(position_controlled=0, du_lo=ONE, du_hi=ONE, **st(rho=0.0))),
                ("plain_beyond_lds_no_workspace", dict(model=QUAD, position_controlled=0, T=51))]
    if fam == "quasi":
        if by_settings:
            out += [("solver_auto", dict(solver=0)), ("solver_active_set", dict(solver=2)), ("solver_tiles", dict(solver=3)),
                    ("solver_out_of_range", dict(solver=4)),
                    ("null_At_and_solver_auto", dict(At=None, solver=0)),
                    ("solver_auto_and_one_sided_u", dict(solver=0, u_hi=None)),
                    ("solver_auto_and_null_settings", dict(solver=0, settings=None))]
        else:
            two = dict(du_lo=ONE, du_hi=ONE)
            out += [("solver_four", dict(solver=4)), ("solver_negative", dict(solver=-1)),
                    ("null_At_and_solver_four", dict(At=None, solver=4)),
                    ("solver_four_and_one_sided_u", dict(solver=4, u_hi=None)),
                    ("active_set_two_boxes", dict(solver=2, **two)), ("tiles_two_boxes", dict(solver=3, **two)),
                    ("active_set_x_bounds", dict(solver=2, x_lo=ONE, x_hi=ONE)),
                    ("tiles_two_boxes_and_rho_zero", dict(solver=3, rho=0.0, **two)),
                    ("tiles_two_boxes_and_unknown_model", dict(solver=3, model=UNKNOWN, **two)),
                    ("active_set_not_position_controlled", dict(solver=2, model=bad)),
                    ("tiles_not_position_controlled", dict(solver=3, model=bad)),
                    ("auto_not_position_controlled", dict(solver=0, model=bad)),
                    ("active_set_beyond_lds", dict(solver=2, T=2000)),
                    ("tiles_beyond_lds_no_workspace", dict(solver=3, T=2000)),
                    ("auto_two_boxes_beyond_lds_no_workspace", dict(solver=0, T=57, **two))]
            if has_ws:
                out += [("tiles_small_workspace", dict(solver=3, T=2000, workspace=WS, workspace_bytes=8))]
    if has_ws and fam != "quasi":
        # a workspace that is given takes the records at any horizon: checked before the model's constants are read
        out += [("misaligned_workspace", dict(workspace=OFF, workspace_bytes=BIG)),
                ("small_workspace", dict(workspace=WS, workspace_bytes=8)),
                ("misaligned_and_small_workspace", dict(workspace=OFF, workspace_bytes=8)),
                ("rho_zero_and_misaligned_workspace", dict(workspace=OFF, workspace_bytes=BIG, **st(rho=0.0))),
                ("unknown_model_with_workspace", dict(model=UNKNOWN, workspace=WS, workspace_bytes=BIG)),
                ("unknown_model_misaligned_workspace", dict(model=UNKNOWN, workspace=OFF, workspace_bytes=BIG)),
                ("param_count_with_workspace", dict(n_params=3, workspace=WS, workspace_bytes=BIG)),
                ("param_count_small_workspace", dict(n_params=3, workspace=WS, workspace_bytes=8))]
        if fam == "solve":
            out += [("not_position_controlled_model_with_workspace", dict(model=bad, workspace=WS, workspace_bytes=BIG)),
                    ("not_position_controlled_model_small_workspace", dict(model=bad, workspace=WS, workspace_bytes=8)),
                    ("not_position_controlled_model_misaligned_workspace",
                     dict(model=bad, workspace=OFF, workspace_bytes=BIG))]
    if has_ws and fam == "quasi":
        # the workspace is used only beyond the LDS horizon (T > 56 on the planar hand), and only checked there
        out += [("beyond_lds_misaligned_workspace", dict(T=80, workspace=OFF, workspace_bytes=BIG)),
                ("beyond_lds_small_workspace", dict(T=80, workspace=WS, workspace_bytes=8)),
                ("beyond_lds_misaligned_and_small_workspace", dict(T=80, workspace=OFF, workspace_bytes=8)),
                ("not_position_controlled_model_with_workspace", dict(model=bad, workspace=WS, workspace_bytes=BIG))]
    return out


def cases():
    """[(entry, case, overrides)], every entry's cases in a fixed order."""
    return [(entry, name, over) for entry in ENTRIES for name, over in entry_cases(entry)]


def _n_params(lib, model):
    n, m, npar = _lib.c_int(), _lib.c_int(), _lib.c_int()
    return npar.value if lib.irs_model_info(model, n, m, npar) == 0 else 1


def call(lib, entry, over):
    """One call of the table: (return code, irs_last_error text)."""
    names = ENTRIES[entry]
    v = dict(BASE)
    v["model"] = BICYCLE if _family(entry) == "descent" else HAND
    v.update(over)
    npar = _n_params(lib, v["model"])
    v.setdefault("n_params", npar)
    v.setdefault("params", _lib.dbl_array([0.1] * npar))
    st = None if v["settings"] is None else _lib.admm_settings(**{**{k: v[k] for k in SCALARS}, **v["settings"]})
    v["settings"] = None if st is None else ctypes.byref(st)
    rc = getattr(lib, entry)(*[v.get(name, ONE) for name in names])
    return rc, lib.irs_last_error().decode("utf-8")


def run(lib):
    """{"<entry>/<case>": [return code, error text]} of the whole table."""
    return {"%s/%s" % (entry, name): list(call(lib, entry, over)) for entry, name, over in cases()}


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(run(_lib.load()), f, indent=0, sort_keys=True)
        f.write("\n")
