"""Calls into the five entries of the unbounded path -- irs_tvlqr_descent, irs_descent_run, irs_tvlqr_descent_batch
(csrc/tvlqr.hip), irs_tvlqr_plan_within_bounds, irs_tvlqr_plan_within_bounds_batch (csrc/iterate.hip) -- that must be
refused BEFORE any launch: every argument check, in every entry, and -- where two checks would fire -- which of them
wins.  Pointers are fake non-null addresses: a refused call dereferences nothing, and no GPU is opened.

cases() is the table, run(lib) its (return code, irs_last_error text) per (entry, case).  The results of the library
as it stood when the single and the batched entries still had a launch path each are
tests/golden/descent_entry_errors.json; tests/test_descent_entries_cpu.py holds every later library to them.
`python -m tests.helpers.descent_entry_cases OUT.json` records the table from the library in the tree (or
IRS_HIP_LIB)."""
import ctypes
import json
import sys

from irs_mpc_amd import _lib

PENDULUM, QUADROTOR, HAND = _lib.MODEL_PENDULUM, _lib.MODEL_QUADROTOR, _lib.MODEL_PLANAR_HAND
UNKNOWN = 99
ONE = 8                 # any non-null address

PROBLEM = ["At", "Bt", "ct", "Q", "Qd", "R", "alpha_R", "xd_trj", "x0"]
OUTPUTS = ["K", "k", "x_new", "u_new", "cost", "info"]
PLAN = ["At", "Bt", "ct", "K", "k", "x_new", "xlo", "xhi", "ulo", "uhi", "flag"]

# entry -> its parameters in order (include/irs_hip.h); irs_descent_run takes the same values in an irs_descent_call
ENTRIES = {
    "irs_tvlqr_descent": ["model", "params", "n_params", "T"] + PROBLEM + OUTPUTS + ["stream"],
    "irs_descent_run": ["call", "stream"],
    "irs_tvlqr_descent_batch": ["model", "params", "n_params", "T", "B"] + PROBLEM + OUTPUTS + ["stream"],
    "irs_tvlqr_plan_within_bounds": ["n", "m", "T"] + PLAN + ["stream"],
    "irs_tvlqr_plan_within_bounds_batch": ["n", "m", "T", "B"] + PLAN + ["stream"],
}

# what a call that would run looks like (never made): every case below overrides at least one of these so that it
# is refused.  "model" stands for (model, params, n_params)
BASE = dict(model=QUADROTOR, T=10, B=3, n=12, m=4, alpha_R=0.5, stream=None)


def _pointers(entry):
    names = ENTRIES[entry] if entry != "irs_descent_run" else PROBLEM + OUTPUTS
    return [p for p in names if p in PROBLEM + OUTPUTS + PLAN and p != "alpha_R"]


def entry_cases(entry):
    """(case name, overrides) of one entry."""
    names = ENTRIES[entry]
    out = [("T_zero", dict(T=0))]
    out += [("null_%s" % p, {p: None}) for p in _pointers(entry)]
    if "B" in names:
        out += [("B_zero", dict(B=0)), ("B_negative", dict(B=-1)), ("B_zero_and_T_zero", dict(B=0, T=0)),
                ("B_zero_and_null_At", dict(B=0, At=None))]
    if "n" in names:
        out += [("n_zero", dict(n=0)), ("n_33", dict(n=33)), ("m_zero", dict(m=0)), ("m_17", dict(m=17)),
                ("n_33_and_null_At", dict(n=33, At=None)), ("T_zero_and_null_flag", dict(T=0, flag=None))]
    else:
        out += [("unknown_model", dict(model=UNKNOWN)), ("negative_model", dict(model=-1)),
                ("param_count", dict(n_params=3)), ("pendulum_param_count", dict(model=PENDULUM, n_params=9)),
                # which check wins
                ("null_At_and_unknown_model", dict(At=None, model=UNKNOWN)),
                ("null_info_and_unknown_model", dict(info=None, model=UNKNOWN)),
                ("T_zero_and_param_count", dict(T=0, n_params=3)),
                ("unknown_model_and_param_count", dict(model=UNKNOWN, n_params=3))]
        if "params" in names:                   # (irs_descent_call holds the parameters themselves)
            out += [("null_params", dict(params=None)), ("null_params_and_T_zero", dict(params=None, T=0))]
        if "B" in names:
            out += [("contact_model", dict(model=HAND)), ("contact_model_and_param_count", dict(model=HAND, n_params=3)),
                    ("contact_model_and_null_params", dict(model=HAND, params=None)),
                    ("contact_model_and_T_zero", dict(model=HAND, T=0)),
                    ("contact_model_and_null_At", dict(model=HAND, At=None))]
    if entry == "irs_descent_run":
        out += [("null_call", dict(call=None))]
    return out


def cases():
    """[(entry, case, overrides)], every entry's cases in a fixed order."""
    return [(entry, name, over) for entry in ENTRIES for name, over in entry_cases(entry)]


def _n_params(lib, model):
    n, m, npar = _lib.c_int(), _lib.c_int(), _lib.c_int()
    return npar.value if lib.irs_model_info(model, n, m, npar) == 0 else 1


def call(lib, entry, over):
    """One call of the table: (return code, irs_last_error text)."""
    v = dict(BASE)
    v.update(over)
    npar = _n_params(lib, v["model"])
    v.setdefault("n_params", npar)
    v.setdefault("params", _lib.dbl_array([0.1] * npar))
    if entry == "irs_descent_run":
        c = _lib.DescentCall()
        c.model, c.n_params, c.T, c.alpha_R = v["model"], v["n_params"], v["T"], v["alpha_R"]
        for i in range(npar):
            c.params[i] = 0.1
        for p in _pointers(entry):
            setattr(c, p, v.get(p, ONE))
        args = [ctypes.byref(c) if v.get("call", ONE) is not None else None, None]
    else:
        args = [v.get(name, ONE) for name in ENTRIES[entry]]
    rc = getattr(lib, entry)(*args)
    return rc, lib.irs_last_error().decode("utf-8")


def run(lib):
    """{"<entry>/<case>": [return code, error text]} of the whole table."""
    return {"%s/%s" % (entry, name): list(call(lib, entry, over)) for entry, name, over in cases()}


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(run(_lib.load()), f, indent=0, sort_keys=True)
        f.write("\n")
