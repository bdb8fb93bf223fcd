"""The argument checks of the five entries of the unbounded path (csrc/tvlqr.hip, csrc/iterate.hip): every refused call
of tests/helpers/descent_entry_cases.py returns the code and the exact irs_last_error text recorded in
tests/golden/descent_entry_errors.json -- from the library as it stood when the single and the batched entries still
had a launch path each.  Which check fires, in what order, under what name and with what numbers is thereby pinned
for all of them.  No GPU is touched: every call of the table is refused before any HIP call."""
import json
import os

import pytest

from tests.helpers import descent_entry_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "descent_entry_errors.json")
REFUSALS = (-1, -3)     # IRS_ERR_INVALID_ARG, _UNSUPPORTED: what an argument check of these entries returns


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
    keys = ["%s/%s" % (entry, name) for entry, name, _ in dc.cases()]
    assert len(keys) == len(set(keys))
    assert sorted(keys) == sorted(golden)
    assert {k.split("/")[0] for k in keys} == set(dc.ENTRIES) and len(dc.ENTRIES) == 5


def test_every_recorded_case_was_refused(golden):
    """The condition the table lives under: no case may reach a launch (its pointers are fake)."""
    for key, (rc, text) in golden.items():
        assert rc != 0 and rc in REFUSALS and text, (key, rc, text)


def test_the_table_has_the_cases_that_pin_the_order(golden):
    """A null pointer beside an unknown model, T = 0 beside a wrong parameter count, the batch's own refusals."""
    for entry in ("irs_tvlqr_descent", "irs_descent_run", "irs_tvlqr_descent_batch"):
        for case in ("null_At_and_unknown_model", "T_zero_and_param_count", "unknown_model", "param_count"):
            assert "%s/%s" % (entry, case) in golden
    for case in ("contact_model", "B_zero", "B_negative", "null_params"):
        assert "irs_tvlqr_descent_batch/" + case in golden
    for entry in ("irs_tvlqr_plan_within_bounds", "irs_tvlqr_plan_within_bounds_batch"):
        for case in ("n_zero", "n_33", "m_zero", "m_17", "T_zero"):
            assert "%s/%s" % (entry, case) in golden
    assert "irs_descent_run/null_call" in golden


@pytest.mark.parametrize("entry", list(dc.ENTRIES))
def test_entry_reproduces_the_recorded_refusals(lib, golden, entry):
    for name, over in dc.entry_cases(entry):
        key = "%s/%s" % (entry, name)
        want = golden[key]
        if want[0] not in REFUSALS:         # never: see above.  Such a call is not made
            pytest.fail("%s is not recorded as refused" % key)
        assert list(dc.call(lib, entry, over)) == want, key
