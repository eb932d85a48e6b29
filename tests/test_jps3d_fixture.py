"""The JPS3D reference runs (tests/golden/jps3d_runs.npz) are self-consistent, and the package exposes
the planner they are the yardstick for."""
import math
import os

import numpy as np
import pytest

import jps3d_checks as J
from golden_io import GOLDEN

# make_golden_jps3d.py: 80 + 40 + 80 + 8 + 4 + 2 random grids and six hand-made cases
N_CASES = 220


@pytest.fixture(scope="module")
def cases():
    return J.cases()


def test_fixture_has_every_group(cases):
    assert len(cases) == N_CASES
    dims = [c["occ"].shape for c in cases]
    for shape, n in [((16, 14, 12), 80), ((21, 15, 11), 40), ((12, 10, 8), 80), ((72, 7, 7), 10), ((40, 30, 30), 4),
                     ((18, 16, 12), 2), ((10, 9, 8), 4)]:
        assert dims.count(shape) == n, shape
    assert sum(c["heuristic"] == "manhattan" for c in cases) == 20
    assert os.path.getsize(os.path.join(GOLDEN, J.FIXTURE)) < 300 * 1024
    # a re-expansion (a pop that overwrites a CLOSED cell) and a failed search, often enough to matter
    assert sum(c["expansions"] > len(c["closed"]) for c in cases) >= 30
    assert sum(len(c["path"]) == 0 for c in cases) >= 5
    # the hand-made cases: start == goal, start occupied, goal occupied, goal sealed in a box
    h = cases[-6:-2]
    assert h[0]["cost"] == 0.0 and len(h[0]["path"]) == 1 and len(h[0]["closed"]) == 1
    assert h[1]["occ"][tuple(h[1]["start"])] and len(h[1]["closed"]) == 1 and math.isinf(h[1]["cost"])
    assert h[2]["occ"][tuple(h[2]["goal"])] and math.isinf(h[2]["cost"])
    g = h[3]["goal"]
    box = h[3]["occ"][g[0] - 1:g[0] + 2, g[1] - 1:g[1] + 2, g[2] - 1:g[2] + 2]
    assert box.sum() == 26 and not h[3]["occ"][tuple(g)] and math.isinf(h[3]["cost"])
    # a jump longer than a wave (64 steps), and a grid whose occupancy does not fit the kernel's LDS staging
    assert [J.decode(v, (72, 7, 7)) for v in cases[-2]["path"]] == [(1, 3, 3), (70, 3, 3)] and cases[-2]["cost"] == 69.0
    assert len(cases[-1]["path"]) >= 2
    assert 40 * 30 * 30 > 32768


def test_fixture_paths_and_costs(cases):
    """Every path segment is a straight 26-direction run whose unit steps pass isCollision; the cost is
    the math.sqrt sum along the path, bit for bit; the CLOSED records agree with the path."""
    for c in cases:
        _, Y, Z = c["occ"].shape
        enc = lambda p: (int(p[0]) * Y + int(p[1])) * Z + int(p[2])  # noqa: E731
        closed = [int(v) for v in c["closed"]]
        assert len(set(closed)) == len(closed) and closed[0] == enc(c["start"]), c["i"]
        assert c["closed_parent"][0] == closed[0] and c["closed_g"][0] == 0.0, c["i"]
        assert c["expansions"] >= len(closed), c["i"]
        if len(c["path"]) == 0:
            assert math.isinf(c["cost"]), c["i"]
            continue
        assert c["path"][0] == enc(c["start"]) and c["path"][-1] == enc(c["goal"]), c["i"]
        assert J.path_cost(c["occ"], c["path"]) == c["cost"], c["i"]
        parent = dict(zip(closed, (int(v) for v in c["closed_parent"])))
        for a, b in zip(c["path"][:-1], c["path"][1:]):
            assert parent[int(b)] == int(a), c["i"]
        assert closed[-1] == enc(c["goal"]), c["i"]


def test_package_exposes_jps3d():
    import torch

    import python_motion_planning_amd as pmp
    from python_motion_planning_amd import _lib, batch

    assert "JPS3D" in pmp.__all__ and issubclass(pmp.JPS3D, pmp.GraphSearcher3D)
    assert "pmp_jps3d_batch" in _lib.SIGNATURES
    assert callable(batch.jps3d_batch)
    env = pmp.Grid3D(10, 9, 8)
    planner = pmp.JPS3D((np.int64(1), np.int64(1), np.int64(1)), (8, 7, 6), env, "manhattan")
    assert str(planner) == "Jump Point Search (JPS) 3D"
    assert planner.start.current == (1, 1, 1) and all(type(v) is int for v in planner.start.current)
    assert planner.start.g == 0.0 and planner.start.h == 18
    if not torch.cuda.is_available():  # no CPU fallback
        with pytest.raises(_lib.PMPError):
            planner.plan()
