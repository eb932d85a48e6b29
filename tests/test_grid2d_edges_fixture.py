"""The CPU oracle (and jps2d_checks.Restated for JPS) reproduces the reference's runs of the nine 2D grid
planners at the sizes test_grid2d_edges_gpu.py leans on it (tests/golden/grid2d_edges.npz,
make_golden_grid2d_edges.py): the 8192-long corridors, 48x383 and 54x307 (the last LDS grid blocks of the
one-query-per-wave and single-query engines), the 8192x48 strip -- bit for bit: cost, path, len(CLOSED) /
len(EXPAND), the CLOSED order; status 4 where the reference raises."""
import os

import numpy as np
import pytest

import grid2d_edges_checks as E
from golden_io import GOLDEN


@pytest.fixture(scope="module")
def cases():
    return E.cases()


def test_fixture_has_every_grid_and_planner(cases):
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f != E.FIXTURE)
    assert os.path.getsize(os.path.join(GOLDEN, E.FIXTURE)) <= largest
    want = [(c[0], c[1], c[2]) for c in E.fixture_case_list()]
    assert [(c["grid"], c["planner"], c["heuristic"]) for c in cases] == want
    for (_, _, _, s, g), c in zip(E.fixture_case_list(), cases):
        assert tuple(c["start"]) == s and tuple(c["goal"]) == g, c["i"]
    dynamic = {"dstar", "lpastar", "dstarlite"}
    for name in ("corridor_x", "corridor_y"):
        assert {c["planner"] for c in cases if c["grid"] == name} >= (set(E.PLANNERS) - {"theta_star", "lazy_theta_star"})
    for name in ("lds_last_48x383", "sq_last_54x307", "strip_8192x48"):
        assert {c["planner"] for c in cases if c["grid"] == name} == set(E.PLANNERS)
    assert {c["planner"] for c in cases if c["grid"] == "corridor_y_theta"} == {"theta_star", "lazy_theta_star"}
    for c in cases:
        o = c["occ"]  # walled: the reference's collision test has no bounds check of its own
        assert o[0].all() and o[-1].all() and o[:, 0].all() and o[:, -1].all(), c["grid"]
        assert ((c["path"] >= 0) & (c["path"] < o.size)).all(), c["i"]
        assert bool(c["closed_sha1"]) == (c["planner"] not in dynamic and not c["raised"]), c["i"]
    # the sizes the launchers switch at (test_grid2d_edges_gpu.py derives them)
    assert E.wave_ldsg_cap(48 * 383, 1) == 64 and E.wave_ldsg_cap(48 * 384, 1) < 64
    assert E.sq_ldsg(54 * 307) and not E.sq_ldsg(54 * 308)


def test_fixture_outcomes_on_the_corridors(cases):
    """The one-shot planners walk the 8,189 (4,093) steps; DStar, LPAStar and DStarLite raise there, which the
    kernels report as status 4."""
    seen = set()
    for c in cases:
        if not c["grid"].startswith("corridor"):
            continue
        steps = 4093 if c["grid"] == "corridor_y_theta" else 8189
        if c["planner"] in ("dstar", "lpastar", "dstarlite"):
            assert c["raised"], (c["grid"], c["planner"])
            seen.add(c["planner"])
        elif c["planner"] == "jps":
            assert c["raised"] in ("", "RecursionError"), c["raised"]
        else:
            assert not c["raised"] and c["cost"] == float(steps), (c["grid"], c["planner"], c["cost"])
            assert len(c["path"]) == (2 if "theta" in c["planner"] else steps + 1), (c["grid"], c["planner"])
    assert seen == {"dstar", "lpastar", "dstarlite"}


def test_oracle_reproduces_every_case(cases):
    n = 0
    for c in cases:
        E.assert_matches_fixture(c, E.oracle_fixture_run(c))
        n += not c["raised"]
    assert n >= 30
    strip = [c for c in cases if c["grid"] == "strip_8192x48" and c["planner"] == "astar"]
    assert len(strip) == 1 and strip[0]["n"] > 250_000 and abs(int(strip[0]["start"][0]) - int(strip[0]["goal"][0])) >= 8180
    assert np.isfinite(strip[0]["cost"])
