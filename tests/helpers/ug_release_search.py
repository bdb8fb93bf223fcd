#!/usr/bin/env python3
"""Seeded CPU search for tests/golden/ug_release_hard.npz: (state, command, du) rows of the planar hand that the
uniform-geometry sample pass cannot settle in its first attempt, classified by the float64 twin
(tests/helpers/ug_release_twin.py):
  kind 1: settles only in the flush's iterations (table rows PDAS + 1 .. PDAS + PDAS_FLUSH);
  kind 2: the release rule never settles it (not within NEVER iterations): the dual steps must finish it.
Searched where such rows were seen: the benchmark's rollout at std 0.3 and random states at std 0.5.  A row is kept only
if it is well inside its class and well conditioned, so that the float32 device takes the same route and the float64
oracle can hold it to the sample pass's f32 tolerance:
  * no |v_i| of the rows it reads lies within MARGIN (relative to max|r|) of the optimality tests;
  * max |lam| / (smallest relative pivot of W on the optimal set) < COND: an f32 solve is good to about eps32 times that,
    and a one-sample `sums` row is held to atol 2e-5 (2e-5 / 6e-8 / |du| ~ 600 at |du| ~ 0.5).

    python tests/helpers/ug_release_search.py [out.npz]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import irs_oracle as orc  # noqa: E402
from tests.helpers import ug_release_twin as tw  # noqa: E402

SEED, NEVER, PER_KIND, PER_STATE = 20240611, 64, 6, 2      # PER_STATE: rows of one kind taken from one state
MARGIN, COND = 1e-4, 100.0


def clear_of_tests(table, W, r, a0, cap):
    """The release iteration from a0 on one sample: True when every bad/good decision on its way has margin."""
    on_t, G_t = table
    scale = np.abs(r).max()
    a = np.array([a0])
    for _ in range(cap):
        v = G_t[a[0]].dot(r)
        if np.abs(v).min() < MARGIN * scale:
            return False
        it, a, _ = tw.iterate(table, r[None], a, 1)
        if it[0]:
            return True
    return True


def conditioning(sys_o, W, r):
    lam = sys_o._dual_exact(W[None], r[None])[0]
    S = np.flatnonzero(lam > 0)
    if len(S) == 0:
        return 0.0
    piv = np.diag(np.linalg.cholesky(W[np.ix_(S, S)])) ** 2 / np.diag(W)[S]
    return np.abs(lam).max() / piv.min()


def search(sys_o, X, U, std, n, rng, found):
    for t in range(X.shape[0]):
        du = (std * rng.normal(size=(n, 4))).astype(np.float32)
        W, R = tw.dual_problems(sys_o, X[t], U[t], du.astype(np.float64))
        table = tw.build_table(W)
        a0 = tw.sweep_guess(W, R)
        it, path, _ = tw.classify(W, R, table=table)
        for kind, idx in ((1, np.flatnonzero(path == tw.PATH_FLUSH)), (2, np.flatnonzero(path == tw.PATH_DUAL))):
            here = 0
            for s in idx:
                if len(found[kind]) >= PER_KIND or here >= PER_STATE:
                    break
                if kind == 2 and tw.iterate(table, R[s:s + 1], a0[s:s + 1], NEVER)[0][0] != 0:
                    continue
                if not clear_of_tests(table, W, R[s], a0[s], NEVER if kind == 2 else tw.PDAS + tw.PDAS_FLUSH):
                    continue
                c = conditioning(sys_o, W, R[s])
                if c >= COND:
                    continue
                here += 1
                found[kind].append((X[t], U[t], du[s], kind))
                print("kind %d: state %s std %.1f sample %d, settles at row %d, |lam|/pivot %.1f" % (
                    kind, t, std, s, it[s], c), flush=True)
        if all(len(found[k]) >= PER_KIND for k in (1, 2)):
            return True
    return False


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), "..", "golden", "ug_release_hard.npz")
    rng = np.random.default_rng(SEED)
    sys_o, x_trj, u_trj = tw.bench_rollout(orc)
    found = {1: [], 2: []}
    if not search(sys_o, x_trj[:50], u_trj, 0.3, 20000, rng, found):
        Xr, Ur = tw.random_states(orc.PlanarHandOracle, rng, 400)
        search(sys_o, Xr, Ur, 0.5, 4000, rng, found)
    rows = found[1] + found[2]
    np.savez(out, x=np.array([r[0] for r in rows]), u=np.array([r[1] for r in rows]),
             du=np.array([r[2] for r in rows], np.float32), kind=np.array([r[3] for r in rows], np.int64))
    print("wrote %s: %d flush-only rows, %d never-settling rows" % (out, len(found[1]), len(found[2])))


if __name__ == "__main__":
    main()
