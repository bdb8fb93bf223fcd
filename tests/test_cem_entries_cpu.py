"""The argument checks of the ten cross-entropy-method entries (csrc/cem_api.hip): every refused call of
tests/helpers/cem_entry_cases.py returns the code and the exact irs_last_error text recorded in
tests/golden/cem_entry_errors.json -- from the library as it stood when each entry still made its checks by hand in
csrc/cem.hip.  Which check fires, in what order, under what name and with what numbers is thereby pinned for all of
them, and so is what the scratch query answers.  No GPU is touched: every call of the table is refused before any HIP
call."""
import json
import os
import re

import pytest

from tests.helpers import cem_entry_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cem_entry_errors.json")
REFUSALS = (-1, -3)         # IRS_ERR_INVALID_ARG, _UNSUPPORTED: what an argument check of this family returns


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from irs_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_and_the_record_hold_the_same_cases(golden):
    keys = ["%s/%s" % (entry, name) for entry, name, _ in cc.cases()]
    assert len(keys) == len(set(keys))
    assert sorted(keys) == sorted(golden["refusals"])
    assert {k.split("/")[0] for k in keys} == set(cc.ENTRIES) and len(cc.ENTRIES) == 10
    sizes = [cc.size_key(c) for c in cc.size_cases()]
    assert len(sizes) == len(set(sizes)) >= 36 and sorted(sizes) == sorted(golden["sizes"])


def test_every_recorded_case_was_refused(golden):
    """The condition the table lives under: no case may reach a launch (its pointers are fake)."""
    for key, (rc, text) in golden["refusals"].items():
        assert rc != 0 and rc in REFUSALS and text, (key, rc, text)


def test_no_recorded_text_names_the_machine(golden):
    for key, (rc, text) in golden["refusals"].items():
        assert not re.search(r"0x[0-9a-f]+|/[a-z]+/|HIP error|hip[A-Z]", text), (key, text)


def test_every_check_of_the_entries_is_recorded(golden):
    """Each distinct refusal text of the entries as they stood in csrc/cem.hip, under each entry that can word it."""
    texts = {(key.split("/")[0], text) for key, (rc, text) in golden["refusals"].items()}

    def said(entry, fragment):
        return any(e == entry and fragment in t for e, t in texts)
    for entry in cc.ENTRIES:
        if "rollout" in entry:
            for fragment in (entry + ": bad argument", "unknown model id 99", "params, got 3"):
                assert said(entry, fragment), (entry, fragment)
            if "quasistatic" in entry:
                assert said(entry, entry + ": model 0 is not position controlled")
        if "refit" in entry:
            assert said(entry, entry + ": need 0 < n_elite <= B") and said(entry, entry + ": null pointer")
        if "stage" in entry:
            for fragment in ("n must be in 1..32", "m must be in 1..16", "T and B must be positive", "t must be in 0..T",
                             "null pointer", "u_t is null at a stage t < T"):
                assert said(entry, entry + ": " + fragment), (entry, fragment)
    assert said("irs_cem_refit_drawn", "must not alias") and not said("irs_cem_refit", "alias")
    for fragment in ("sizes must be positive", "null pointer", "B T m too large for one launch"):
        assert said("irs_cem_candidates", "irs_cem_candidates: " + fragment), fragment
    for fragment in ("null call struct", "T, B and n_descents must be positive", "need 0 < n_elite <= B",
                     "null problem pointer", "the quasistatic cost needs Qd", "null output / scratch pointer",
                     "model 0 is not position controlled", "scratch 3071 < 3072 bytes", "scratch 0 < 3072 bytes"):
        assert said("irs_cem_iterate", "irs_cem_iterate: " + fragment), fragment
    assert said("irs_cem_iterate", "unknown model id 99") and said("irs_cem_iterate", "params, got 3")


@pytest.mark.parametrize("entry", list(cc.ENTRIES))
def test_entry_reproduces_the_recorded_refusals(lib, golden, entry):
    for name, over in cc.entry_cases(entry):
        key = "%s/%s" % (entry, name)
        want = golden["refusals"][key]
        if want[0] not in REFUSALS:         # never: see above.  Such a call is not made
            pytest.fail("%s is recorded as accepted" % key)
        assert list(cc.call(lib, entry, over)) == want, key


def test_scratch_query_answers_what_was_recorded(lib, golden):
    assert cc.sizes(lib) == golden["sizes"]
