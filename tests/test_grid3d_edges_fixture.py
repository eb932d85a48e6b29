"""The CPU oracle reproduces the reference's runs of the seven 3D grid planners at the sizes where the
kernels change behaviour (tests/golden/grid3d_edges.npz: 33x32x32 and 65x32x32, above the LDS occupancy
thresholds; 256-long grids; a goal sealed in a box), bit for bit: every call's cost, path and
len(CLOSED) / len(EXPAND), and the CLOSED order.  test_grid3d_edges_gpu.py holds the kernels to both."""
import math
import os

import numpy as np
import pytest

import grid3d_edges_checks as E
from golden_io import GOLDEN


@pytest.fixture(scope="module")
def cases():
    return E.cases()


def test_fixture_has_every_group(cases):
    assert os.path.getsize(os.path.join(GOLDEN, E.FIXTURE)) < 300 * 1024
    every = set(E.STATIC + E.DYNAMIC)
    for group, dims, planners in [("rand33", {(33, 32, 32)}, every), ("big65", {(65, 32, 32)}, {"astar", "theta_star", "dstar", "lpastar"}),
                                  ("thin", {(256, 4, 4), (4, 256, 4), (4, 4, 256)}, every), ("sealed", {(33, 32, 32)}, every)]:
        sel = [c for c in cases if c["group"] == group]
        assert {c["occ"].shape for c in sel} == dims, group
        assert {c["planner"] for c in sel} == planners, group
    assert sum(c["planner"] == "astar" and c["heuristic"] == "manhattan" for c in cases) == 2
    # above the thresholds the launchers switch at: 1024 words (astar3d.hip), 2048 words (dstar3d.hip, lpa3d.hip)
    assert 33 * 32 * 32 > 1024 * 32 and 65 * 32 * 32 > 2048 * 32
    for c in cases:
        o = c["occ"]  # walled: the reference's isCollision has no bounds test of its own
        assert o[0].all() and o[-1].all() and o[:, 0].all() and o[:, -1].all() and o[:, :, 0].all() and o[:, :, -1].all()
        assert len(c["cost"]) == (E.R if c["planner"] in E.DYNAMIC else 1)
        for p in c["paths"]:
            assert ((p >= 0) & (p < o.size)).all(), c["i"]


def test_fixture_no_path_cases(cases):
    """Each planner's own no-path result, on the cut 4x256x4 grid and on the sealed goal."""
    n = 0
    for c in cases:
        # the thin grid drawn at density 0.1 (the others at 0.03): its 2x2 free cross-section is cut
        cut = c["group"] == "sealed" or (c["group"] == "thin" and c["occ"][1:-1, 1:-1, 1:-1].mean() > 0.06)
        if c["group"] == "sealed":
            g = c["goal"]
            box = c["occ"][g[0] - 1:g[0] + 2, g[1] - 1:g[1] + 2, g[2] - 1:g[2] + 2]
            assert box.sum() == 26 and not c["occ"][tuple(g)]
        _, Y, Z = c["occ"].shape
        goal = (int(c["goal"][0]) * Y + int(c["goal"][1])) * Z + int(c["goal"][2])
        reached = len(c["paths"][0]) > 0 and c["paths"][0][-1] == goal
        if c["group"] in ("thin", "sealed"):
            assert reached == (not cut), (c["i"], c["planner"])
        if not reached:
            n += 1
            if c["planner"] in E.STATIC:
                assert math.isinf(c["cost"][0]) and len(c["paths"][0]) == 0 and c["n"][0] > 0
            elif c["planner"] == "dstar":  # extractPath stops at the parentless start
                assert c["cost"][0] == 0.0 and len(c["paths"][0]) == 1
            else:  # extractPath: no candidate (0.0) or the 100000-step guard
                assert c["cost"][0] in (0.0, 100000.0) and len(c["paths"][0]) == 0
    assert n >= 4
    assert any(c["planner"] == "lpastar" and c["cost"][0] == 100000.0 for c in cases)


def test_fixture_rounds(cases):
    """DStar3D's rounds block a voxel of the planned path and one outside the grid; LPAStar3D's block a
    path voxel and toggle it back."""
    for c in cases:
        X, Y, Z = c["occ"].shape
        if c["planner"] == "dstar" and c["group"] in ("rand33", "big65"):
            b = c["blocks"]
            assert (int(b[0, 0, 0]) * Y + int(b[0, 0, 1])) * Z + int(b[0, 0, 2]) in c["paths"][0], c["i"]
            assert b[0, 1, 0] == X and b[1, 1, 0] == -1, c["i"]
        if c["planner"] == "lpastar":
            ch = c["changes"]
            assert ch[0, 3] == 1 and ch[1, 3] == 0 and (ch[0, :3] == ch[1, :3]).all(), c["i"]
            if c["group"] in ("rand33", "big65"):
                assert (int(ch[0, 0]) * Y + int(ch[0, 1])) * Z + int(ch[0, 2]) in c["paths"][0], c["i"]


def test_oracle_reproduces_every_case(cases):
    for c in cases:
        E.assert_matches_fixture(c, E.oracle_run(c))


def test_oracle_endpoint_outside_the_grid():
    """An endpoint outside the grid is not searched (include/pmp.h): no path at inf; a start inside the
    grid is the one CLOSED cell; pushes, pops, expansions, max heap = 1, 1, n_expanded, 1.  (The oracle
    used to index its per-cell arrays with such a start.)"""
    from oracle import oracle as O

    occ = np.zeros((5, 4, 3), np.uint8)
    for lazy in (None, False, True):
        for s, g, s_in in [((-1, 1, 1), (2, 2, 2), 0), ((5, 1, 1), (2, 2, 2), 0), ((1, 1, 1), (2, 4, 2), 1),
                           ((1, 1, 1), (2, 2, -3), 1), ((300, 0, 0), (0, 0, 256), 0), ((7, 7, 7), (7, 7, 7), 0)]:
            r = O.astar3d(occ, s, g) if lazy is None else O.theta3d(occ, s, g, lazy=lazy)
            assert r["status"] == 1 and math.isinf(r["cost"]) and len(r["path_cells"]) == 0, (lazy, s, g)
            assert r["n_expanded"] == s_in and list(r["expand_cells"]) == [(s[0] * 4 + s[1]) * 3 + s[2]] * s_in
            assert (r["n_push"], r["n_pop"], r["n_iter"], r["max_heap"]) == (1, 1, s_in, 1), (lazy, s, g)
