"""Why the primal-dual iteration of the uniform-geometry sample pass (csrc/smooth_ug.hip, ug_pdas) releases ONE row per
iteration: the float64 twin (tests/helpers/ug_release_twin.py) on the benchmark's own inputs.

On states 0, 25 and 49 of the benchmark's rollout, 4096 samples each at std 0.3:
  * the rule settles >= 95 % of the samples within 4 table rows and >= 99.5 % within 6;
  * every settled sample carries the multipliers of the oracle's exact dual active-set method;
  * the rule it replaced (flip every non-optimal row at once) leaves >= 10 % unsettled after 4 rows -- those were parked.
And the fixture tests/golden/ug_release_hard.npz (tests/helpers/ug_release_search.py) still holds what it was searched
for: rows that settle only in the flush's iterations and rows the rule never settles.
"""
import os

import numpy as np
import pytest

from oracle import irs_oracle as orc
from tests.helpers import ug_release_twin as tw

SEED = 5
STATES, N, STD = (0, 25, 49), 4096, 0.3
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "ug_release_hard.npz")


@pytest.fixture(scope="module")
def problems():
    sys_o, x_trj, u_trj = tw.bench_rollout(orc)
    rng = np.random.default_rng(SEED)
    out = []
    for t in STATES:
        du = (STD * rng.normal(size=(N, 4))).astype(np.float32).astype(np.float64)
        W, R = tw.dual_problems(sys_o, x_trj[t], u_trj[t], du)
        out.append((W, R, tw.build_table(W)))
    return sys_o, out


def test_release_rule_settles_what_the_flip_rule_parked(problems):
    sys_o, probs = problems
    its, flips = [], []
    for W, R, table in probs:
        it, path, lam = tw.classify(W, R, table=table)        # the device's caps; `it` counts through the flush
        its.append(it)
        exact = sys_o._dual_exact(np.repeat(W[None], len(R), 0), R)
        got = it > 0
        err = np.abs(lam[got] - exact[got]).max(1) / np.maximum(np.abs(exact[got]).max(1), np.abs(R[got]).max(1))
        print("settled %d of %d, max |lam - exact| relative %.2e" % (got.sum(), len(R), err.max()))
        assert err.max() <= 1e-9
        flips.append(tw.classify(W, R, rule="flip", pdas=4, flush=0, table=table)[0])       # the caps it had
    it, flip = np.concatenate(its), np.concatenate(flips)
    within4 = np.mean((it > 0) & (it <= 4))
    within6 = np.mean((it > 0) & (it <= 6))
    parked_flip = np.mean(flip == 0)
    print("release rule: %.2f %% within 4 rows, %.2f %% within 6; flip rule parks %.2f %%" % (
        100 * within4, 100 * within6, 100 * parked_flip))
    assert within4 >= 0.95
    assert within6 >= 0.995
    assert parked_flip >= 0.10


def test_fixture_rows_keep_their_class():
    """kind 1: settled by the flush's iterations alone; kind 2: never settled by the rule (64 iterations)."""
    sys_o = orc.PlanarHandOracle(0.1)
    f = np.load(FIXTURE)
    assert (f["kind"] == 1).sum() >= 4 and (f["kind"] == 2).sum() >= 4
    for x, u, du, kind in zip(f["x"], f["u"], f["du"], f["kind"]):
        W, R = tw.dual_problems(sys_o, x, u, du[None].astype(np.float64))
        table = tw.build_table(W)
        it, path, _ = tw.classify(W, R, table=table)
        if kind == 1:
            assert path[0] == tw.PATH_FLUSH and tw.PDAS < it[0] <= tw.PDAS + tw.PDAS_FLUSH
        else:
            assert path[0] == tw.PATH_DUAL
            assert tw.iterate(table, R, tw.sweep_guess(W, R), 64)[0][0] == 0
