"""Calls into the ten cross-entropy-method entries of the C ABI (csrc/cem_api.hip) that must be refused BEFORE any
launch: every argument check, in every entry, and -- where two checks would fire -- which of them wins.  Pointers are
fake non-null addresses: a refused call dereferences nothing, and no GPU is opened.

cases() is the table, run(lib) its (return code, irs_last_error text) per (entry, case); size_cases() / sizes(lib) are
irs_cem_iterate_scratch_bytes on a few dozen (T, m, B, n_elite).  The results of the library as it stood while the
entries still checked by hand in csrc/cem.hip are tests/golden/cem_entry_errors.json; tests/test_cem_entries_cpu.py
holds every later library to them.  `python -m tests.helpers.cem_entry_cases OUT.json` records both tables from the
library in the tree (or IRS_HIP_LIB).

Every check of those entries, and a case that reaches it (R = each of the four rollout entries, Rq = the two
quasistatic ones, S = both stage entries):
  R   "bad argument"                               R/T_zero, R/B_negative, R/null_x0, R/null_u_cand | null_std, ...
  R   irs_load_params: unknown model               R/unknown_model
  R   irs_load_params: parameter count, null       R/param_count, R/null_params
  Rq  "model %d is not position controlled"        Rq/not_position_controlled
  Rq  "bad argument" for a missing Qd              Rq/null_Qd
  irs_cem_refit        "need 0 < n_elite <= B"     irs_cem_refit/n_elite_zero, /n_elite_B_plus_1, /T_zero, /m_zero
  irs_cem_refit        "null pointer"              irs_cem_refit/null_u_cand, /null_costs, /null_elite_idx, ...
  irs_cem_refit_drawn  "need 0 < n_elite <= B"     irs_cem_refit_drawn/n_elite_zero, /n_elite_B_plus_1, /B_zero
  irs_cem_refit_drawn  "null pointer"              irs_cem_refit_drawn/null_u_mean, /null_std, /null_u_new, ...
  irs_cem_refit_drawn  the alias check             irs_cem_refit_drawn/alias_u_new_u_mean, /alias_u_new_std,
                                                   /alias_std_new_u_mean, /alias_std_new_std, /alias_u_new_std_new,
                                                   /alias_partial_overlap
  irs_cem_candidates   "sizes must be positive"    irs_cem_candidates/T_zero, /m_negative, /B_zero
  irs_cem_candidates   "null pointer"              irs_cem_candidates/null_u_mean, /null_std, /null_u_cand
  irs_cem_candidates   "B T m too large ..."       irs_cem_candidates/beyond_one_launch
  S   "n must be in 1..32"                         S/n_zero, S/n_33
  S   "m must be in 1..16"                         S/m_zero, S/m_17
  S   "T and B must be positive"                   S/T_zero, S/B_zero
  S   "t must be in 0..T"                          S/t_negative, S/t_beyond_T
  S   "null pointer" (shared pointers)             S/null_x, S/null_Q, S/null_R, S/null_xd_trj, S/null_costs
  S   "u_t is null at a stage t < T"               S/null_u_t
  S   "null pointer" (the candidate source)        S/null_u_cand | null_u_mean, null_std; at t == T, where a null u_t
                                                   is accepted: S/last_stage_null_u_t_then_null_source
  irs_cem_iterate  "null call struct"              irs_cem_iterate/null_call
  irs_cem_iterate  "T, B and n_descents ..."       irs_cem_iterate/T_zero, /B_zero, /n_descents_zero
  irs_cem_iterate  "need 0 < n_elite <= B"         irs_cem_iterate/n_elite_zero, /n_elite_B_plus_1
  irs_cem_iterate  "null problem pointer"          irs_cem_iterate/null_Q, /null_R, /null_xd_trj, /null_x0, /null_u_trj0,
                                                   /null_std0
  irs_cem_iterate  "the quasistatic cost needs Qd" irs_cem_iterate/quasistatic_null_Qd (a position-controlled model)
  irs_cem_iterate  "null output / scratch pointer" irs_cem_iterate/null_u_hist, /null_std_hist, /null_x_hist,
                                                   /null_cost_hist, /null_scratch
  irs_cem_iterate  irs_model_info: unknown model   irs_cem_iterate/unknown_model
  irs_cem_iterate  irs_load_params                 irs_cem_iterate/param_count
  irs_cem_iterate  "not position controlled"       irs_cem_iterate/quasistatic_not_position_controlled
  irs_cem_iterate  "scratch %zu < %zu bytes"       irs_cem_iterate/scratch_one_byte_short, /scratch_zero
The names joined by _and_ are the double faults: the first named is the one the parent reports."""
import ctypes
import json
import sys

from irs_mpc_amd import _lib

PEND, BOX = _lib.MODEL_PENDULUM, _lib.MODEL_BOX_PIVOT_EXACT     # not position controlled (n 2, m 1); position controlled (m 2)
UNKNOWN = 99
INT_MAX = 2 ** 31 - 1

POINTERS = ["u_cand", "u_mean", "std", "x0", "Q", "Qd", "R", "xd_trj", "costs", "elite_idx", "u_new", "std_new", "x", "u_t",
            "u_trj0", "std0", "u_hist", "std_hist", "x_hist", "cost_hist", "scratch"]
ADDR = {name: 0x100000 * (i + 1) for i, name in enumerate(POINTERS)}      # distinct, 1 MiB apart: nothing aliases

MODEL = ["model", "params", "n_params"]
DRAW = ["u_mean", "std", "seed", "iter", "sample_offset"]
# entry -> its parameters in order (include/irs_hip.h)
ENTRIES = {
    "irs_cem_rollout_costs": MODEL + ["T", "B", "u_cand", "x0", "Q", "R", "xd_trj", "costs", "stream"],
    "irs_cem_rollout_costs_quasistatic": MODEL + ["T", "B", "u_cand", "x0", "Q", "Qd", "R", "xd_trj", "costs", "stream"],
    "irs_cem_rollout_costs_drawn": MODEL + ["T", "B"] + DRAW + ["x0", "Q", "R", "xd_trj", "costs", "stream"],
    "irs_cem_rollout_costs_quasistatic_drawn": MODEL + ["T", "B"] + DRAW + ["x0", "Q", "Qd", "R", "xd_trj", "costs",
                                                                           "stream"],
    "irs_cem_refit": ["T", "m", "B", "n_elite", "u_cand", "costs", "elite_idx", "u_new", "std_new", "stream"],
    "irs_cem_refit_drawn": ["T", "m", "B", "n_elite"] + DRAW + ["costs", "elite_idx", "u_new", "std_new", "stream"],
    "irs_cem_candidates": ["T", "m", "B"] + DRAW + ["u_cand", "stream"],
    "irs_cem_values_stage": ["n", "m", "T", "B", "t", "x", "u_cand", "Q", "R", "xd_trj", "u_t", "costs", "stream"],
    "irs_cem_values_stage_drawn": ["n", "m", "T", "B", "t", "x"] + DRAW + ["Q", "R", "xd_trj", "u_t", "costs", "stream"],
    "irs_cem_iterate": ["call", "stream"],
}
ITERATE_POINTERS = ("Q", "Qd", "R", "xd_trj", "x0", "u_trj0", "std0", "u_hist", "std_hist", "x_hist", "cost_hist", "scratch")

# what a call that would run looks like (never made): every case below overrides at least one of these so that it
# is refused.  "model" stands for (model, params, n_params); scratch_short = bytes taken off what the size query asks
BASE = dict(ADDR, T=5, B=300, m=1, n=2, t=2, n_elite=7, seed=7, iter=1, sample_offset=0, stream=None,
            n_descents=3, quasistatic=0, scratch_short=0)


def _source(entry):
    """The pointers of the entry's candidate source."""
    return ["u_mean", "std"] if "u_mean" in ENTRIES[entry] else ["u_cand"]


def _rollout_cases(entry):
    quasi = "quasistatic" in entry
    src = _source(entry)
    nulls = src + ["x0", "Q", "R", "xd_trj", "costs"] + (["Qd"] if quasi else [])
    out = [("T_zero", dict(T=0)), ("T_negative", dict(T=-3)), ("B_zero", dict(B=0)), ("B_negative", dict(B=-1))]
    out += [("null_" + p, {p: None}) for p in nulls]
    out += [("unknown_model", dict(model=UNKNOWN)), ("param_count", dict(n_params=3)), ("null_params", dict(params=None)),
            # which of two faults is reported
            ("T_zero_and_unknown_model", dict(T=0, model=UNKNOWN)),
            ("null_costs_and_param_count", dict(costs=None, n_params=3)),
            ("null_%s_and_null_params" % src[-1], {src[-1]: None, "params": None}),
            ("unknown_model_and_param_count", dict(model=UNKNOWN, n_params=1, params=None))]
    if quasi:
        out += [("not_position_controlled", dict(model=PEND)),
                ("null_Qd_and_not_position_controlled", dict(model=PEND, Qd=None)),
                ("B_zero_and_not_position_controlled", dict(model=PEND, B=0)),
                ("param_count_and_not_position_controlled", dict(model=PEND, n_params=3)),
                ("null_params_and_not_position_controlled", dict(model=PEND, params=None))]
    return out


def _refit_cases(entry):
    drawn = entry.endswith("_drawn")
    src = _source(entry)
    out = [("T_zero", dict(T=0)), ("T_negative", dict(T=-1)), ("m_zero", dict(m=0)), ("m_negative", dict(m=-2)),
           ("B_zero", dict(B=0)), ("B_negative", dict(B=-300)),
           ("n_elite_zero", dict(n_elite=0)), ("n_elite_negative", dict(n_elite=-7)),
           ("n_elite_B_plus_1", dict(n_elite=301)), ("n_elite_one_B_zero", dict(n_elite=1, B=0))]
    out += [("null_" + p, {p: None}) for p in src + ["costs", "elite_idx", "u_new", "std_new"]]
    out += [("n_elite_zero_and_null_costs", dict(n_elite=0, costs=None)),
            ("T_zero_and_null_%s" % src[0], {"T": 0, src[0]: None}),
            ("n_elite_B_plus_1_and_null_std_new", dict(n_elite=301, std_new=None))]
    if drawn:
        len_bytes = 8 * BASE["T"] * BASE["m"]
        out += [("alias_u_new_u_mean", dict(u_new=ADDR["u_mean"])), ("alias_u_new_std", dict(u_new=ADDR["std"])),
                ("alias_std_new_u_mean", dict(std_new=ADDR["u_mean"])), ("alias_std_new_std", dict(std_new=ADDR["std"])),
                ("alias_u_new_std_new", dict(u_new=ADDR["std_new"])),
                ("alias_swapped", dict(u_new=ADDR["std"], std_new=ADDR["u_mean"])),
                ("alias_partial_overlap", dict(u_new=ADDR["u_mean"] + len_bytes - 8)),
                ("alias_partial_overlap_from_below", dict(std_new=ADDR["std"] - len_bytes + 8)),
                ("alias_partial_overlap_of_outputs", dict(std_new=ADDR["u_new"] + 8)),
                ("n_elite_zero_and_alias", dict(n_elite=0, u_new=ADDR["u_mean"])),
                ("null_std_new_and_alias", dict(std_new=None, u_new=ADDR["u_mean"])),
                ("null_costs_and_alias", dict(costs=None, std_new=ADDR["std"]))]
    return out


def _candidates_cases(entry):
    huge = dict(B=INT_MAX, T=1024)                  # 2^41 elements: beyond 2^31 - 1 blocks of 256
    return [("T_zero", dict(T=0)), ("T_negative", dict(T=-5)), ("m_zero", dict(m=0)), ("m_negative", dict(m=-1)),
            ("B_zero", dict(B=0)), ("B_negative", dict(B=-1)),
            ("null_u_mean", dict(u_mean=None)), ("null_std", dict(std=None)), ("null_u_cand", dict(u_cand=None)),
            ("beyond_one_launch", huge),
            ("B_zero_and_null_u_cand", dict(B=0, u_cand=None)),
            ("null_std_and_beyond_one_launch", dict(std=None, **huge)),
            ("m_zero_and_beyond_one_launch", dict(m=0, **huge))]


def _stage_cases(entry):
    src = _source(entry)
    last = dict(t=BASE["T"], u_t=None)              # the stage without a control: a null u_t is accepted there
    out = [("n_zero", dict(n=0)), ("n_negative", dict(n=-2)), ("n_33", dict(n=33)),
           ("m_zero", dict(m=0)), ("m_17", dict(m=17)),
           ("T_zero", dict(T=0, t=0)), ("T_negative", dict(T=-1, t=0)), ("B_zero", dict(B=0)), ("B_negative", dict(B=-1)),
           ("t_negative", dict(t=-1)), ("t_beyond_T", dict(t=BASE["T"] + 1))]
    out += [("null_" + p, {p: None}) for p in ["x", "Q", "R", "xd_trj", "costs", "u_t"] + src]
    out += [("first_stage_null_u_t", dict(t=0, u_t=None)), ("stage_before_last_null_u_t", dict(t=BASE["T"] - 1, u_t=None))]
    out += [("last_stage_null_u_t_then_null_" + p, dict(last, **{p: None})) for p in src + ["costs"]]
    out += [("last_stage_null_u_t_then_n_33", dict(last, n=33)),
            # which of two faults is reported
            ("n_33_and_m_17", dict(n=33, m=17)), ("m_zero_and_T_zero", dict(m=0, T=0, t=0)),
            ("T_zero_and_t_negative", dict(T=0, t=-1)), ("B_zero_and_t_beyond_T", dict(B=0, t=BASE["T"] + 1)),
            ("t_beyond_T_and_null_x", dict(t=BASE["T"] + 1, x=None)), ("t_negative_and_null_u_t", dict(t=-1, u_t=None)),
            ("null_x_and_null_u_t", dict(x=None, u_t=None)),
            ("null_u_t_and_null_%s" % src[0], {"u_t": None, src[0]: None}),
            ("null_Q_and_null_%s" % src[-1], {"Q": None, src[-1]: None}),
            ("m_17_and_null_%s" % src[0], {"m": 17, src[0]: None})]
    return out


def _iterate_cases(entry):
    quasi = dict(model=BOX, m=2, quasistatic=1)     # the quasistatic cost where it is served
    out = [("null_call", dict(call=None)),
           ("T_zero", dict(T=0)), ("T_negative", dict(T=-1)), ("B_zero", dict(B=0)), ("B_negative", dict(B=-2)),
           ("n_descents_zero", dict(n_descents=0)), ("n_descents_negative", dict(n_descents=-1)),
           ("n_elite_zero", dict(n_elite=0)), ("n_elite_negative", dict(n_elite=-1)), ("n_elite_B_plus_1", dict(n_elite=301))]
    out += [("null_" + p, {p: None}) for p in ITERATE_POINTERS if p != "Qd"]
    out += [("quasistatic_null_Qd", dict(quasi, Qd=None)),
            ("unknown_model", dict(model=UNKNOWN)), ("unknown_model_quasistatic", dict(model=UNKNOWN, quasistatic=1)),
            ("param_count", dict(n_params=3)), ("param_count_zero", dict(n_params=0)),
            ("quasistatic_not_position_controlled", dict(quasistatic=1)),
            ("quasistatic_flag_two_not_position_controlled", dict(quasistatic=2)),
            ("scratch_one_byte_short", dict(scratch_short=1)), ("scratch_zero", dict(scratch_short=None)),
            ("quasistatic_scratch_one_byte_short", dict(quasi, scratch_short=1)),
            # the plain cost never reads Qd: the call gets past that check, and the next fault is reported
            ("plain_null_Qd_then_scratch_one_byte_short", dict(Qd=None, scratch_short=1)),
            ("plain_null_Qd_then_unknown_model", dict(Qd=None, model=UNKNOWN)),
            # which of two faults is reported
            ("B_zero_and_n_elite_zero", dict(B=0, n_elite=0)), ("n_descents_zero_and_null_Q", dict(n_descents=0, Q=None)),
            ("n_elite_B_plus_1_and_null_std0", dict(n_elite=301, std0=None)),
            ("null_x0_and_quasistatic_null_Qd", dict(quasi, x0=None, Qd=None)),
            ("quasistatic_null_Qd_and_null_u_hist", dict(quasi, Qd=None, u_hist=None)),
            ("quasistatic_null_Qd_and_not_position_controlled", dict(quasistatic=1, Qd=None)),
            ("null_scratch_and_unknown_model", dict(scratch=None, model=UNKNOWN)),
            ("null_cost_hist_and_scratch_zero", dict(cost_hist=None, scratch_short=None)),
            ("unknown_model_and_param_count", dict(model=UNKNOWN, n_params=3)),
            ("unknown_model_and_scratch_zero", dict(model=UNKNOWN, scratch_short=None)),
            ("param_count_and_not_position_controlled", dict(quasistatic=1, n_params=3)),
            ("param_count_and_scratch_one_byte_short", dict(n_params=3, scratch_short=1)),
            ("not_position_controlled_and_scratch_one_byte_short", dict(quasistatic=1, scratch_short=1))]
    return out


def entry_cases(entry):
    """(case name, overrides) of one entry."""
    if "rollout" in entry:
        return _rollout_cases(entry)
    if "refit" in entry:
        return _refit_cases(entry)
    if "stage" in entry:
        return _stage_cases(entry)
    return _candidates_cases(entry) if entry == "irs_cem_candidates" else _iterate_cases(entry)


def cases():
    """[(entry, case, overrides)], every entry's cases in a fixed order."""
    return [(entry, name, over) for entry in ENTRIES for name, over in entry_cases(entry)]


def _n_params(lib, model):
    n, m, npar = _lib.c_int(), _lib.c_int(), _lib.c_int()
    return npar.value if lib.irs_model_info(model, n, m, npar) == 0 else 1


def _struct(lib, v, npar):
    c = _lib.CemIterateCall()
    c.model, c.n_params = v["model"], v["n_params"]
    for i in range(min(npar, 12)):
        c.params[i] = 0.1
    c.T, c.B, c.n_elite, c.n_descents, c.quasistatic = v["T"], v["B"], v["n_elite"], v["n_descents"], v["quasistatic"]
    c.seed, c.iter0 = v["seed"], v["iter"]
    for p in ITERATE_POINTERS:
        setattr(c, p, v[p])
    short = v["scratch_short"]
    c.scratch_bytes = 0 if short is None else lib.irs_cem_iterate_scratch_bytes(v["T"], v["m"], v["B"], v["n_elite"]) - short
    return c


def call(lib, entry, over):
    """One call of the table: (return code, irs_last_error text)."""
    v = dict(BASE)
    v["model"] = BOX if "quasistatic" in entry else PEND
    v.update(over)
    npar = _n_params(lib, v["model"])
    v.setdefault("n_params", npar)
    v.setdefault("params", _lib.dbl_array([0.1] * npar))
    if entry == "irs_cem_iterate" and "call" not in v:
        c = _struct(lib, v, npar)
        v["call"] = ctypes.byref(c)
    rc = getattr(lib, entry)(*[v[name] for name in ENTRIES[entry]])
    return rc, lib.irs_last_error().decode("utf-8")


def run(lib):
    """{"<entry>/<case>": [return code, error text]} of the whole table."""
    return {"%s/%s" % (entry, name): list(call(lib, entry, over)) for entry, name, over in cases()}


def size_cases():
    """[(T, m, B, n_elite)] of the scratch query: sizes on both sides of a 256-byte boundary of either part, and
    arguments that make it answer 0."""
    out = [(30, 1, B, e) for B in (1, 31, 32, 33, 300, 500, 50000) for e in (1, 64, 65)]
    out += [(T, m, 300, 7) for T in (1, 5, 1000) for m in (1, 2, 16)]
    out += [(0, 1, 300, 7), (5, 0, 300, 7), (5, 1, 0, 7), (5, 1, 300, 0), (-1, 1, 300, 7), (5, -1, 300, 7),
            (5, 1, -300, 7), (5, 1, 300, -7), (0, 0, 0, 0), (5, 1, 300, 301), (5, 1, INT_MAX, INT_MAX)]
    return out


def size_key(case):
    return "T%d/m%d/B%d/n_elite%d" % case


def sizes(lib):
    """{key: irs_cem_iterate_scratch_bytes}."""
    return {size_key(case): lib.irs_cem_iterate_scratch_bytes(*case) for case in size_cases()}


if __name__ == "__main__":
    lib = _lib.load()
    with open(sys.argv[1], "w") as f:
        json.dump({"refusals": run(lib), "sizes": sizes(lib)}, f, indent=0, sort_keys=True)
        f.write("\n")
