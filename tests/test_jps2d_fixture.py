"""The JPS reference runs (tests/golden/jps2d_runs.npz) are reproduced by the collapsed, iterative form
of jump() that csrc/jps2d.hip implements (jps2d_checks.Restated), their paths are jump-point chains,
and the package exposes the planner they are the yardstick for."""
import os

import numpy as np
import pytest

import jps2d_checks as J
from golden_io import GOLDEN

# make_golden_jps2d.py: 40 + 39 x 8 random, 2 readme, 4 + 4 + 1 rooms, 6 + 3 + 4 hand-made, 6 on the C2 grid
N_CASES = 382


@pytest.fixture(scope="module")
def grids():
    return J.grids()


def test_fixture_has_every_group(grids):
    assert sum(len(g["cases"]) for g in grids) == N_CASES
    assert os.path.getsize(os.path.join(GOLDEN, J.FIXTURE)) < 700 * 1024
    by = {g["name"]: g for g in grids}
    assert by["random00"]["occ"].shape == (64, 45) and len(by["random00"]["cases"]) == 40
    rnd = [g for g in grids if g["name"].startswith("random")]
    assert len(rnd) == 40 and all(g["occ"].shape[1] % 32 for g in rnd)
    assert {37, 45, 63} <= {g["occ"].shape[1] for g in rnd}
    for g in grids:  # border walls: where equality with the reference is claimed
        o = g["occ"]
        assert o[0].all() and o[-1].all() and o[:, 0].all() and o[:, -1].all(), g["name"]
    cases = [c for g in grids for c in g["cases"]]
    assert sum(c["heuristic"] == "manhattan" for c in cases) >= 100
    assert sum(not c["found"] for c in cases) >= 12
    assert sum(c["found"] and len(c["path"]) == 1 for c in cases) >= 40  # start == goal
    assert sum(c["found"] and c["n_closed"] == 2 and len(c["path"]) == 2 for c in cases) >= 30  # adjacent
    r = by["readme"]["cases"][0]
    assert (float(r["cost"]), len(r["path"]), r["n_closed"]) == (53.45584412271572, 10, 10)
    r = by["room200"]["cases"][0]
    assert (float(r["cost"]), r["n_closed"]) == (238.0071426749364, 3)
    for name in ("room300x77", "room77x300"):  # legs of more than 128 steps
        W, H = by[name]["occ"].shape
        legs = [max(abs(a // H - b // H), abs(a % H - b % H)) for c in by[name]["cases"]
                for a, b in zip(c["path"][:-1], c["path"][1:])]
        assert max(legs) > 128, name
    sq = by["squeeze"]
    assert sq["occ"][5, 6] and sq["occ"][6, 5] and not sq["occ"][5, 5] and not sq["occ"][6, 6]
    assert sq["cases"][1]["found"] and len(sq["cases"][1]["path"]) == 2  # through the squeeze in one step
    assert not sq["cases"][3]["found"] and sq["occ"][tuple(sq["cases"][3]["goal"])]
    assert sq["cases"][4]["found"] and sq["occ"][tuple(sq["cases"][4]["start"])]
    co = by["corridor"]["cases"]
    assert all(c["found"] for c in co) and len(co[0]["path"]) >= 6  # two ends, four turns
    c2 = by["c2"]
    assert c2["occ"].shape == (1024, 1024) and len(c2["cases"]) == 6 and all(c["closed"] is None for c in c2["cases"])


def compare(occ, c, r):
    tag = (c["i"], occ.shape)
    assert r["found"] == c["found"], tag
    assert np.float64(r["cost"]).view(np.int64) == np.float64(c["cost"]).view(np.int64), tag
    assert list(r["path"]) == [int(v) for v in c["path"]], tag
    assert (r["pushes"], r["pops"], r["max_heap"]) == (c["pushes"], c["pops"], c["max_heap"]), tag
    assert len(r["closed"]) == c["n_closed"], tag
    assert J.closed_digest(r["closed"], r["parent"], r["g"]) == c["digest"], tag
    if c["closed"] is not None:
        assert r["closed"] == [int(v) for v in c["closed"]], tag
        assert r["parent"] == [int(v) for v in c["closed_parent"]], tag
        assert np.array_equal(np.array(r["g"], np.float64).view(np.int64), c["closed_g"].view(np.int64)), tag


def test_restatement_reproduces_the_reference(grids):
    """Cost, path, CLOSED order, parents, g and the heap counts, bit for bit, on every stored grid."""
    n = 0
    for g in grids:
        if not g["stored"]:
            continue
        rs = J.Restated(g["occ"])
        for c in g["cases"]:
            compare(g["occ"], c, rs.plan(c["start"], c["goal"], c["heuristic"]))
            n += 1
    assert n == N_CASES - 6


def test_restatement_reproduces_the_reference_c2(grids):
    """The same on the six queries of the 1024^2 grid, whose CLOSED records are compared by digest."""
    g = next(g for g in grids if not g["stored"])
    rs = J.Restated(g["occ"])
    for c in g["cases"]:
        compare(g["occ"], c, rs.plan(c["start"], c["goal"], c["heuristic"]))


def test_fixture_paths_are_jump_point_chains(grids):
    for g in grids:
        H = g["occ"].shape[1]
        for c in g["cases"]:
            if not c["found"]:
                assert len(c["path"]) == 0 and c["cost"] == 0.0, c["i"]
                continue
            enc = lambda p: int(p[0]) * H + int(p[1])  # noqa: E731
            assert c["path"][0] == enc(c["goal"]) and c["path"][-1] == enc(c["start"]), c["i"]
            assert J.check_chain(g["occ"], c["path"]) == c["cost"], c["i"]
            if c["closed"] is not None:
                parent = dict(zip((int(v) for v in c["closed"]), (int(v) for v in c["closed_parent"])))
                assert len(parent) == c["n_closed"] and int(c["closed"][0]) == enc(c["start"]), c["i"]
                for a, b in zip(c["path"][:-1], c["path"][1:]):
                    assert parent[int(a)] == int(b), c["i"]


def test_package_exposes_jps():
    import torch

    import python_motion_planning_amd as pmp
    from python_motion_planning_amd import _lib, batch

    assert "JPS" in pmp.__all__ and issubclass(pmp.JPS, pmp.AStar)
    assert "pmp_jps2d_batch" in _lib.SIGNATURES
    assert callable(batch.jps2d_batch) and callable(pmp.JPS.plan_batch)
    planner = pmp.JPS((5, 5), (45, 25), pmp.Grid(51, 31), "manhattan")
    assert str(planner) == "Jump Point Search(JPS)"
    assert planner.start.current == (5, 5) and planner.goal.current == (45, 25)
    if not torch.cuda.is_available():  # no CPU fallback
        with pytest.raises(_lib.PMPError):
            planner.plan()
