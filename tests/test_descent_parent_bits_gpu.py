"""The Riccati descent and the tail-plan test compute the bits they computed when their single-problem and batched
kernels were separate sources: every array of tests/helpers/descent_parent_cases.py -- K, k, x_new, u_new, cost, info
of irs_tvlqr_descent per problem and of irs_tvlqr_descent_batch on every path of the backward pass, of the single
entry on a contact model, and the four histories of irs_iterate without bounds, with bounds that never bind (the info
row comes from the plan test) and with one that does -- has the shape and the SHA-256 recorded in
tests/golden/descent_parent_bits.json from that earlier library.  Equality of digests is equality of bit patterns,
NaNs included: there is no tolerance.  Where the record holds the values too, a mismatch names its first entry."""
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import descent_parent_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "descent_parent_bits.json")
HAND = "planar_hand-T%d" % pc.HAND_T


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()     # fails loudly if the HIP library is missing
    return irs_mpc_amd


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def hold(case, got, want):
    """Every array of `got` against its record; all of the record's arrays are there."""
    want = {k: v for k, v in want.items() if k != "inputs"}
    assert sorted(got) == sorted(want), case
    for name, a in got.items():
        w = want[name]
        assert list(a.shape) == w["shape"], (case, name, a.shape, w["shape"])
        if pc.digest(a) != w["sha256"]:
            where = ""
            if "values" in w:
                ref = np.array(w["values"], dtype=a.dtype).reshape(a.shape)
                bad = np.argwhere(a.view(np.uint64 if a.dtype == np.float64 else a.dtype)
                                  != ref.view(np.uint64 if a.dtype == np.float64 else a.dtype))
                where = ": first at %s, got %r, recorded %r" % (tuple(bad[0]), a[tuple(bad[0])], ref[tuple(bad[0])])
            pytest.fail("%s %s differs from the recorded bits%s" % (case, name, where))


def test_the_record_holds_these_cases(golden):
    cases = [pc.case_id(name, B, T) for name, B, T, _ in pc.DESCENT_CASES] + [HAND] + ["iterate-" + r for r in pc.ITERATE_RUNS]
    assert sorted(golden) == sorted(cases)
    assert os.path.getsize(GOLDEN) < 100 * 1024


@pytest.mark.parametrize("name,B,T,path", pc.DESCENT_CASES, ids=[pc.case_id(*c[:3]) for c in pc.DESCENT_CASES])
def test_descents_single_and_batched(amd, golden, name, B, T, path):
    case = pc.case_id(name, B, T)
    got = pc.run_descents(amd, name, B, T)
    assert (got["batch/info"] == 0).all(), (case, got["batch/info"])        # the recorded problems all solve
    hold(case, got, golden[case])


def test_descent_of_a_contact_model(amd, golden):
    inputs = {k: np.array(v["values"], float).reshape(v["shape"]) for k, v in golden[HAND]["inputs"].items()}
    hold(HAND, pc.run_hand(amd, inputs), golden[HAND])


def test_iterate_histories(amd, golden):
    got = pc.run_iterates(amd)
    rows = {run: got["iterate-" + run]["info_hist"] for run in pc.ITERATE_RUNS}
    print(rows)
    # what the three runs are there for: the row written by the descent's launch, by the plan test with flag 0, and
    # with flag 1
    assert (rows["free"] == 0).all() and (rows["wide"] == 0).all()
    assert rows["u_cut"][0, 2] == 1 and rows["u_cut"][0, 0] == 0
    for run in pc.ITERATE_RUNS:
        hold("iterate-" + run, got["iterate-" + run], golden["iterate-" + run])
