"""IrsLqr._replay, the one copy of the loop's bookkeeping (append to the three lists, stop after max_iterations, adopt,
count) that `_iterate_fused`, `IrsLqrBatch.iterate` and the verbose loop share: on given rows of irs_iterate's info
history it leaves `x_trj_lst`, `u_trj_lst`, `cost_lst`, `iter`, the adopted triple and the exception exactly where the
loop of `_iterate_fused` left them when it still did the bookkeeping itself.  The expected values below were recorded
by running that loop's body, as it stood then, on the same rows.  No GPU and no library: the object under test is made
with object.__new__ and carries only what the bookkeeping touches."""
import numpy as np
import pytest

from irs_mpc_amd.irs_lqr import IrsLqr

OK = [0] * 8
RICCATI = [3, 0, 0, 0, 0, 0, 0, 0]              # [0]: the backward pass failed
SMOOTHING = [0, 2, 0, 0, 0, 0, 0, 0]            # [1]: two smoothing solves failed
BOX_UNSOLVED = [0, 0, 1, 0, 7, 1, 0, 0]         # [2] bounded descent ran, [5] and did not converge
BOX_SOLVED = [0, 0, 1, 0, 7, 0, 0, 0]
ROWS = {"clean": [OK, BOX_SOLVED, OK], "fail_first": [RICCATI, OK, OK], "fail_middle_smoothing": [OK, SMOOTHING, OK],
        "fail_middle_box": [OK, BOX_UNSOLVED, OK], "long": [OK, OK, BOX_SOLVED, OK, OK]}
MAX_ITERATIONS = 2
T_FAILED = "TV_LQR failed. Optimization problem is not solved."
S_FAILED = ("randomized-smoothing least squares is rank deficient (Gram matrix not positive definite; need more samples "
            "or a non-zero std)")

# (history, iter before) -> descents logged, iter after, descent adopted (None: the start triple), exception
EXPECTED = {
    ("clean", 1): ([0, 1, 2], 3, 1, None),
    ("fail_first", 1): ([], 1, None, (ValueError, T_FAILED)),
    ("fail_middle_smoothing", 1): ([0], 2, 0, (ValueError, S_FAILED)),
    ("fail_middle_box", 1): ([0], 2, 0, (ValueError, T_FAILED)),
    ("long", 1): ([0, 1, 2], 3, 1, None),
    ("clean", 3): ([0], 3, None, None),
    ("fail_first", 3): ([], 3, None, (ValueError, T_FAILED)),
    ("fail_middle_smoothing", 3): ([0], 3, None, None),
    ("fail_middle_box", 3): ([0], 3, None, None),
    ("long", 3): ([0], 3, None, None),
}


def bare(it):
    s = object.__new__(IrsLqr)
    s.x_trj_lst, s.u_trj_lst, s.cost_lst = ["x start"], ["u start"], [-1.0]
    s.iter, s.x_trj, s.u_trj, s.cost = it, "x start", "u start", -1.0
    return s


@pytest.mark.parametrize("name,it", sorted(EXPECTED))
def test_replay_keeps_the_books_as_the_fused_loop_did(name, it):
    rows = np.array(ROWS[name], np.int32)
    D = len(rows)
    xs = [np.full((2, 1), 10.0 + i) for i in range(D)]
    us = [np.full((1, 1), 20.0 + i) for i in range(D)]
    cs = np.array([100.5 + i for i in range(D)])
    logged, iter_after, adopted, exc = EXPECTED[(name, it)]
    s = bare(it)
    got = s._replay(xs, us, cs, [s._fused_failure(row) for row in rows], MAX_ITERATIONS)
    if exc is None:
        assert got is None
    else:
        assert type(got) is exc[0] and str(got) == exc[1]
    assert len(s.x_trj_lst) == len(s.u_trj_lst) == len(s.cost_lst) == 1 + len(logged)
    assert s.x_trj_lst[0] == "x start" and s.u_trj_lst[0] == "u start" and s.cost_lst[0] == -1.0
    for j, i in enumerate(logged, 1):
        assert s.x_trj_lst[j] is xs[i] and s.u_trj_lst[j] is us[i]
        assert type(s.cost_lst[j]) is float and s.cost_lst[j] == 100.5 + i
    assert s.iter == iter_after
    if adopted is None:
        assert (s.x_trj, s.u_trj, s.cost) == ("x start", "u start", -1.0)
    else:
        assert s.x_trj is xs[adopted] and s.u_trj is us[adopted]
        assert type(s.cost) is float and s.cost == 100.5 + adopted


def test_the_failure_is_whatever_the_caller_put_there():
    """IrsLqrBatch hands its status texts through: the first one comes back, the lists hold what came before."""
    s = bare(1)
    xs, us = [np.zeros(1), np.ones(1), np.ones(1)], [np.zeros(1)] * 3
    assert s._replay(xs, us, [1.0, 2.0, 3.0], [None, "stopped", "later"], 5) == "stopped"
    assert len(s.x_trj_lst) == 2 and s.iter == 2 and s.x_trj is xs[0] and s.cost == 1.0
