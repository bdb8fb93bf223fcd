"""The launch geometry of the sample pass (irs_smooth_geometry, the planner the launch itself uses) against the
restated sample loops of oracle/smooth_cases.py: every sample of every shape has exactly one reader, and the cases
of tests/test_smooth_accounting_gpu.py reach the geometry they name and can see a lost sample.  No GPU."""
import collections
import ctypes
import os

import numpy as np
import pytest

from oracle import smooth_cases as sc

TS = list(range(1, 65)) + [80, 100, 128, 200, 1024]
# dense where the plans change shape (a few wave trips), then a stride prime to every tile size, every multiple of 1024 with
# its neighbours
NS = sorted(set(list(range(1, 321)) + list(range(321, 20000, 251)) + [v + e for v in range(1024, 20481, 1024) for e in (-1, 0, 1)]
                + list(range(20000, 300001, 9973)) + [300000]))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from irs_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.load()


class general_kernel:
    """IRS_UG=0 for the calls inside (read per call by the query and by the launch)."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.before = os.environ.get("IRS_UG")
        if self.on:
            os.environ["IRS_UG"] = "0"

    def __exit__(self, *a):
        if self.on:
            if self.before is None:
                os.environ.pop("IRS_UG", None)
            else:
                os.environ["IRS_UG"] = self.before


def query(lib, model_id, mode, T, N, rng, buf=(ctypes.c_int * 8)()):
    assert lib.irs_smooth_geometry(model_id, mode, T, N, int(rng), buf) == 0
    return tuple(buf[:7])


def as_geom(g):
    from irs_mpc_amd import _lib
    return dict(family=_lib.SMOOTH_FAMILIES[g[0]], block=g[1], nblk=g[2], chunk0=g[3], chunk=g[4], wg0_rr=g[5],
                branch=_lib.SMOOTH_PLANS[g[6]])


def test_query_is_what_the_python_binding_reports(lib):
    from irs_mpc_amd import device as dev
    assert dev.smooth_geometry(9, sc.ZERO_ORDER_B, 65, 897) == as_geom(query(lib, 9, sc.ZERO_ORDER_B, 65, 897, False))
    assert dev.smooth_geometry(0, 0, 3, 1025)["block"] == 1024 and dev.smooth_geometry(0, 0, 3, 1025, rng=True)["block"] == 256
    buf = (ctypes.c_int * 8)()
    assert lib.irs_smooth_geometry(0, 0, 0, 10, 0, buf) == -1 and lib.irs_smooth_geometry(0, 7, 1, 10, 0, buf) == -1
    assert lib.irs_smooth_geometry(99, 0, 1, 10, 0, buf) != 0 and lib.irs_smooth_geometry(0, 0, 1, 10, 0, None) == -1
    # IRS_UG is read per call
    with general_kernel(True):
        assert dev.smooth_geometry(8, sc.ZERO_ORDER_B, 1, 449)["family"] == sc.PARKED
    assert dev.smooth_geometry(8, sc.ZERO_ORDER_B, 1, 449)["family"] == sc.UG


def test_every_shape_gives_every_sample_one_reader(lib):
    """>= 1e5 shapes: all registered models x 3 modes x supplied / device-drawn (+ the planar hand's general kernels
    under IRS_UG=0).  Combinations the planner cannot tell apart are swept once: they are grouped by the geometry
    they get on a probe set, and the grouping is part of what is asserted."""
    g = np.random.default_rng(0)
    probe = [(int(t), int(n)) for t, n in zip(g.choice(TS, 160), g.choice(NS, 160))]
    combos = [(mid, mode, rng, False) for mid in range(11) for mode in range(3) for rng in (False, True)]
    combos += [(8, mode, rng, True) for mode in (sc.FIRST_ORDER, sc.ZERO_ORDER_B) for rng in (False, True)]
    classes = collections.OrderedDict()
    for c in combos:
        with general_kernel(c[3]):
            sig = tuple(query(lib, c[0], c[1], T, N, c[2]) for T, N in probe)
        classes.setdefault((sig, c[2] and sig[0][0] == 0), []).append(c)
    queried, table, empties, seen = 0, collections.Counter(), collections.Counter(), {}
    buf = (ctypes.c_int * 8)()
    geometry, ws_bytes = lib.irs_smooth_geometry, lib.irs_smooth_workspace_bytes
    for (sig, _), members in classes.items():
        mid, mode, rng, general = members[0]
        P4 = (lib.irs_sums_len(mid, mode) + 3) // 4 * 4
        with general_kernel(general):
            for T in TS:
                assert T * 4 <= 4096                                    # the arrival counters
                for N in NS:
                    assert geometry(mid, mode, T, N, rng, buf) == 0
                    key = (buf[0], buf[1], buf[2], buf[3], buf[4], buf[5], buf[6], N, rng)
                    # the partial rows were sized by a plan made with rng = true: (T, nblk, P) floats behind the
                    # counters (4096 bytes) and the nominal steps (T x 32 doubles)
                    assert 4096 + T * 256 + T * key[2] * P4 * 4 <= ws_bytes(mid, mode, T, N), (members[0], T, N, key)
                    n_empty = seen.get(key)
                    if n_empty is None:
                        geom = as_geom(key)
                        n_empty = 0
                        if geom["family"] != sc.UG:
                            beg, end = sc.wg_ranges(geom, N)
                            # in order, no overlap, no gap, all of [0, N): each range starts where the last one ended
                            # (or past N: an empty workgroup)
                            assert beg[0] == 0 and end[-1] == N and (np.diff(beg) > 0).all() \
                                and (end[:-1] == np.minimum(beg[1:], N)).all(), (geom, N)
                            n_empty = int((end <= beg).sum())
                        assert sc.tiles(sc.owners(geom, N, rng), N), (members[0], T, N, geom)
                        seen[key] = n_empty
                    queried += 1
                    table[(key[0], key[6])] += len(members)
                    if n_empty:
                        empties[(key[0], key[6])] += len(members)
    from irs_mpc_amd import _lib
    shapes = sum(table.values())
    table = {(_lib.SMOOTH_FAMILIES[k[0]], _lib.SMOOTH_PLANS[k[1]]): v for k, v in table.items()}
    empties = {(_lib.SMOOTH_FAMILIES[k[0]], _lib.SMOOTH_PLANS[k[1]]): v for k, v in empties.items()}
    print("\n%d shapes queried on the full grid (%d classes of the %d combinations, which stand for %d shapes), "
          "%d distinct (geometry, N)" % (queried, len(classes), len(combos), shapes, len(seen)))
    for k in sorted(table):
        print("  %-20s %-6s %9d shapes, %d with an empty workgroup" % (k[0], k[1], table[k], empties.get(k, 0)))
    assert queried >= 100000
    assert {k[0] for k in table} == {sc.LIGHT, sc.HEAVY, sc.GRAM, sc.WAVE_DEALT, sc.PARKED, sc.UG}
    # the case table of oracle/smooth_cases.py has no "nominal cost" plan and no empty workgroup because no shape gets
    # one; a planner that starts to produce them needs cases for them
    assert not any(k[1] == "cost" for k in table) and not empties, (table, empties)


def test_reader_count_sees_a_wrong_deal():
    """The restated loops are not trivially satisfied: the faults the accounting tests exist for break `owners`."""
    geom = dict(family=sc.PARKED, block=256, nblk=2, chunk0=448, chunk=512, wg0_rr=1, branch="trips")
    assert (sc.reader_count(sc.owners(geom, 897), 897) == 1).all()
    # (any wg0_rr covers the range -- the loops run until their blocks are past s_end -- it only shifts the balance)
    assert sc.tiles(sc.owners(dict(geom, wg0_rr=2), 897), 897)
    # block_of without the three-wave stride: the last wave still sits out after wg0_rr trips, the others keep 4 k + w
    # (a plan that gives the nominal step two trips; with one, the two deals coincide)
    geom = dict(geom, chunk0=640, chunk=320)
    assert sc.tiles(sc.owners(geom, 897), 897)
    own = sc.owners(dict(geom, wg0_rr=sc.NEVER), 897)
    keep = ~((own["wg"] == 0) & (own["wave"] == 3) & (own["trip"] >= 1))
    assert not sc.tiles({k: v[keep] for k, v in own.items()}, 897)
    ug = dict(family=sc.UG, block=512, nblk=2, chunk0=0, chunk=0, wg0_rr=sc.NEVER, branch="none")
    assert sc.tiles(sc.owners(ug, 5000), 5000)
    # the uniform-geometry numbering: workgroup 1's waves numbered 8 b + w instead of 8 b - 1 + w
    own = sc.owners(ug, 5000)
    bad = dict(own, start=np.where(own["wg"] == 1, own["start"] + 64, own["start"]),
               stop=np.where(own["wg"] == 1, np.minimum(own["stop"] + 64, 5000), own["stop"]))
    assert not sc.tiles(bad, 5000) and (sc.reader_count(bad, 5000) != 1).any()
    # a tail slot of the four-per-lane loop that is not zeroed reads its clamped row once more
    light = dict(family=sc.LIGHT, block=1024, nblk=1, chunk0=2048, chunk=2048, wg0_rr=sc.NEVER, branch="none")
    own = sc.owners(light, 1025)
    tail = own["stop"] <= own["start"]
    assert tail.any() and sc.tiles(own, 1025)
    unzeroed = dict(own, start=np.where(tail, 1024, own["start"]), stop=np.where(tail, 1025, own["stop"]))
    assert sc.reader_count(unzeroed, 1025)[1024] > 1


@pytest.mark.parametrize("cid", list(sc.CASES))
def test_case_reaches_its_geometry_and_sees_a_lost_sample(lib, cid):
    from irs_mpc_amd import device as dev
    c = sc.CASES[cid]
    mid, n, m, contact = sc.MODELS[c["model"]]
    with general_kernel(sc.needs_general_kernel(c)):
        geoms = {src: dev.smooth_geometry(mid, c["mode"], c["T"], c["N"], src == "r") for src in c["sources"]}
    for src, geom in geoms.items():
        why = sc.admit(c, geom, c["N"])
        assert why is None, why
        assert (sc.reader_count(sc.owners(geom, c["N"], src == "r"), c["N"]) == 1).all()
    assert 16 * c["N"] < 2 ** 24
    geom = geoms.get("s") or geoms["r"]
    if c["mode"] == sc.FIRST_ORDER:
        if contact:
            # all-zero du: N equal addends per entry; the bound of the comparison with the N = 64 launch,
            # (trips per lane + 10) 2^-24, must stay a tenth below what one lost sample changes, 1 / N
            assert (sc.trips_per_lane(geom, c["N"]) + 10) * 2.0 ** -24 < 0.1 / c["N"]
        elif "s" in c["sources"]:
            pairs, visible, weakest = sc.weakest_jacobian_swap(c, geom)
            print("%s: %d of %d boundary swaps change the sum of Jacobians; the smallest by %.3g of the block" % (
                cid, visible, pairs, weakest))
            if pairs:
                assert visible >= 1
                assert sc.JAC_BOUND[geom["family"]] <= 0.1 * weakest, (sc.JAC_BOUND[geom["family"]], weakest)
        return
    if "s" not in c["sources"]:
        return
    seen, weakest = sc.weakest_mutation(c, geom, ts=sorted({0, c["T"] - 1}))
    print("%s: every fault at a boundary sample changes the exact blocks: %s; smallest effect on z df': %.3g" % (
        cid, seen, weakest))
    assert seen
    # the device comparison of this block may never allow more than a tenth of what one faulty sample changes
    assert sc.zdf_bound(geom["family"], c["mode"], c["N"]) <= 0.1 * weakest, (sc.zdf_bound(geom["family"], c["mode"], c["N"]), weakest)
