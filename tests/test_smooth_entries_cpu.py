"""The argument checks of the fifteen sample-pass entries (csrc/smooth_api.hip): every refused call of
tests/helpers/smooth_entry_cases.py returns the code and the exact irs_last_error text recorded in
tests/golden/smooth_entry_errors.json -- from the library as it stood when each entry still marshalled and checked by
hand.  Which check fires, in what order, under what name and with what numbers is thereby pinned for all of them, and
so is what the four size queries answer.  No GPU is touched: every call of the table is refused before any HIP call.
(The sweep of irs_smooth_geometry over every model, mode and shape is tests/test_smooth_geometry_cpu.py, unchanged.)"""
import json
import os
import re

import pytest

from tests.helpers import smooth_entry_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "smooth_entry_errors.json")
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
    keys = ["%s/%s" % (entry, name) for entry, name, _ in sc.cases()]
    assert len(keys) == len(set(keys))
    assert sorted(keys) == sorted(golden["refusals"])
    assert {k.split("/")[0] for k in keys} == set(sc.ENTRIES) and len(sc.ENTRIES) == 15
    sizes = [sc.size_key(c) for c in sc.size_cases()]
    assert len(sizes) == len(set(sizes)) >= 36 and sorted(sizes) == sorted(golden["sizes"])


def test_every_recorded_case_was_refused(golden):
    """The condition the table lives under: no case may reach a launch (its pointers are fake)."""
    for key, (rc, text) in golden["refusals"].items():
        assert rc != 0 and rc in REFUSALS and text, (key, rc, text)


def test_no_recorded_number_depends_on_the_machine():
    """The uniform-geometry family sizes its grid by the CU count: its shapes here fit one workgroup on any device."""
    from irs_mpc_amd import _lib
    shapes = [(model, mode, N) for model, mode, T, N, B, env in sc.size_cases() if not env]
    for _, _, over in sc.cases():
        v = dict(sc.BASE, **over)
        if not v["env"]:
            shapes.append((v["model"], v["mode"], v["N"]))
    ug = [s for s in shapes if s[0] == _lib.MODEL_PLANAR_HAND_EXACT and s[1] in (sc.FIRST, sc.ZB)]
    assert len(ug) >= 20 and all(N <= 448 for _, _, N in ug), ug


def test_no_recorded_text_names_the_machine(golden):
    for key, (rc, text) in golden["refusals"].items():
        assert not re.search(r"0x[0-9a-f]+|/[a-z]+/|HIP error|hip[A-Z]", text), (key, text)


@pytest.mark.parametrize("entry", list(sc.ENTRIES))
def test_entry_reproduces_the_recorded_refusals(lib, golden, entry):
    for name, over in sc.entry_cases(entry):
        key = "%s/%s" % (entry, name)
        want = golden["refusals"][key]
        if want[0] not in REFUSALS:         # never: see above.  Such a call is not made
            pytest.fail("%s is recorded as accepted" % key)
        assert list(sc.call(lib, entry, over)) == want, key


def test_size_queries_answer_what_was_recorded(lib, golden):
    assert sc.sizes(lib) == golden["sizes"]
