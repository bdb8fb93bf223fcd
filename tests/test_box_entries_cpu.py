"""The argument checks of the fourteen bounded-ADMM entries (csrc/boxqp_api.hip): every refused call of
tests/helpers/box_entry_cases.py returns the code and the exact irs_last_error text recorded in
tests/golden/box_entry_errors.json -- from the library as it stood when each entry still made its checks by hand.
Which check fires, in what order, under what name and with what numbers is thereby pinned for all of them.  No GPU is
touched: every call of the table is refused before any HIP call."""
import json
import os

import pytest

from tests.helpers import box_entry_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "box_entry_errors.json")
REFUSALS = (-1, -3, -4)     # IRS_ERR_INVALID_ARG, _UNSUPPORTED, _WORKSPACE: what an argument check returns


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
    keys = ["%s/%s" % (entry, name) for entry, name, _ in bc.cases()]
    assert len(keys) == len(set(keys))
    assert sorted(keys) == sorted(golden)
    assert {k.split("/")[0] for k in keys} == set(bc.ENTRIES) and len(bc.ENTRIES) == 14


def test_every_recorded_case_was_refused(golden):
    """The condition the table lives under: no case may reach a launch (its pointers are fake)."""
    for key, (rc, text) in golden.items():
        assert rc != 0 and rc in REFUSALS and text, (key, rc, text)


@pytest.mark.parametrize("entry", list(bc.ENTRIES))
def test_entry_reproduces_the_recorded_refusals(lib, golden, entry):
    for name, over in bc.entry_cases(entry):
        key = "%s/%s" % (entry, name)
        want = golden[key]
        if want[0] == 0:                    # never: see above.  Such a call is not made
            pytest.fail("%s is recorded as accepted" % key)
        assert list(bc.call(lib, entry, over)) == want, key
