"""RRT-Connect without a device: the fixture of reference runs holds the cases the feature is held to,
the sequential restatement of the kernel's arithmetic (rrt_connect_checks.plan) reproduces every one
of them bit for bit, and the feature is exposed through every layer."""
import inspect

import numpy as np
import pytest

import rrt_connect_checks as C
from python_motion_planning_amd import batch

CASES, Z = C.cases()
LDS_NODES = batch.rrt_connect_lds_nodes()  # nodes per tree the kernel keeps in LDS


def _sizes(c):
    return len(c["tree0"]), len(c["tree1"])


def test_fixture_covers_the_cases():
    assert [(c["kind"], c["map"], c["seed"], c["sample_num"], c["max_dist"], c["rate"]) for c in CASES] == (
        [("readme", "readme", s, 10000, 0.5, 0.05) for s in range(16)]
        + [("c3", "c3", s, 10000, 8.0, 0.05) for s in range(3)] + [("c3long", "c3", 0, 10000, 0.5, 0.05)]
        + [("rate", "readme", s, 10000, 0.5, 0.5) for s in (0, 1)] + [("never", "readme", s, 400, 0.5, 0.05) for s in (0, 1)]
        + [("few", "readme", 0, 20, 0.5, 0.05), ("short", "readme", 0, 10000, 0.5, 0.05)])
    by = {}
    for c in CASES:
        by.setdefault(c["kind"], []).append(c)
    sizes = [sum(_sizes(c)) for c in by["readme"]]
    assert (min(sizes), max(sizes)) == (109, 282)
    assert all(tuple(c["start"]) == (18, 8) and tuple(c["goal"]) == (37, 18) for k in ("readme", "rate", "few") for c in by[k])
    assert all(tuple(c["start"]) == (5, 5) and tuple(c["goal"]) == (505, 505) for k in ("c3", "c3long") for c in by[k])
    assert all(100 <= sum(_sizes(c)) <= 140 for c in by["c3"])
    long_ = by["c3long"][0]
    assert (sum(_sizes(long_)), len(long_["path"]), long_["coll"]) == (1872, 1610, 8799)
    # ... the case whose trees leave the kernel's LDS share; the README cases stay inside it
    assert 64 <= LDS_NODES < min(_sizes(long_))
    assert all(max(_sizes(c)) <= LDS_NODES for c in by["readme"])
    for c in by["never"]:
        assert tuple(c["goal"]) == (27, 13) and not c["found"] and _sizes(c)[1] == 1 and c["iters"] == 400
    assert not by["few"][0]["found"] and by["few"][0]["iters"] == 20 and min(_sizes(by["few"][0])) > 1
    short = by["short"][0]
    assert tuple(short["goal"]) == (18, 9) and sum(_sizes(short)) == 5 and len(short["path"]) == 4
    # both orientations at the end
    assert {c["forward"] for c in by["readme"]} == {0, 1}
    for c in CASES:
        assert C.stream(c)[c["draws"]] == c["next"]
        assert c["draws"] <= 3 * c["iters"] <= 3 * c["sample_num"]
        assert c["parent0"][0] == 0 and c["parent1"][0] == 0
        assert tuple(c["tree0"][0]) == (*c["start"], 0.0) and tuple(c["tree1"][0]) == (*c["goal"], 0.0)
        if c["found"]:
            b0, b1 = c["boundary"]
            assert np.array_equal(c["tree0"][b0, :2], c["tree1"][b1, :2])
            assert c["cost"] == c["tree0"][b0, 2] + c["tree1"][b1, 2]
            assert c["n_expand"] == sum(_sizes(c))
            assert tuple(c["path"][0]) == tuple(c["start"]) and tuple(c["path"][-1]) == tuple(c["goal"])
            # the closing approach lands exactly: no degenerate last segment
            assert np.hypot(*(c["path"][1:] - c["path"][:-1]).T).min() > 1e-9
        else:
            assert c["cost"] == 0 and list(c["boundary"]) == [-1, -1] and len(c["path"]) == 0


@pytest.mark.parametrize("i", range(len(CASES)))
def test_restatement_reproduces_reference(i):
    """Both trees, parents, the orientation, the meeting node, cost, path, iterations, draws and the
    number of isCollision calls: equal, not close."""
    c = CASES[i]
    rnd = C.stream(c)
    r = C.plan(c["map"], c["start"], c["goal"], rnd.tolist(), c["sample_num"], max_dist=c["max_dist"], rate=c["rate"])
    assert r["status"] == (C.FOUND if c["found"] else C.NO_PATH)
    for t in (0, 1):
        x, y, g, par = r["tree"][t]
        assert len(x) == len(c[f"tree{t}"])
        assert np.array_equal(np.array(par, np.int32), c[f"parent{t}"])
        assert np.array_equal(np.column_stack([x, y, g]), c[f"tree{t}"])
    assert r["forward"] == c["forward"] and r["boundary"] == list(c["boundary"])
    assert r["iters"] == c["iters"] and r["collision_tests"] == c["coll"]
    assert r["draws"] == c["draws"] and rnd[r["draws"]] == c["next"]
    assert r["cost"] == c["cost"]
    if c["found"]:
        assert np.array_equal(np.array(r["path"], np.float64), c["path"])
    else:
        assert r["path"] is None


def test_restatement_overflows():
    """A tree capacity below the run's needs stops with status 3, a short path_cap with status 2."""
    c = CASES[0]
    kw = dict(max_dist=c["max_dist"], rate=c["rate"])
    r = C.plan(c["map"], c["start"], c["goal"], C.stream(c).tolist(), c["sample_num"], cap=32, **kw)
    assert r["status"] == C.CAP_OVERFLOW and max(len(r["tree"][0][0]), len(r["tree"][1][0])) == 32
    r = C.plan(c["map"], c["start"], c["goal"], C.stream(c).tolist(), c["sample_num"], path_cap=len(c["path"]) - 1, **kw)
    assert r["status"] == C.PATH_OVERFLOW and r["cost"] == c["cost"]


# ---- exposure: each of these fails without the feature --------------------------------------------------
def test_exported_and_subclass():
    import python_motion_planning_amd as pmp

    assert "RRTConnect" in pmp.__all__
    assert issubclass(pmp.RRTConnect, pmp.RRT) and not issubclass(pmp.RRTConnect, pmp.RRTStar)
    p = pmp.RRTConnect((18, 8), (37, 18), C.env_of("readme"))
    assert str(p) == "RRT-Connect" and (p.max_dist, p.sample_num, p.goal_sample_rate, p.delta) == (0.5, 10000, 0.05, 0.5)
    sig = inspect.signature(pmp.RRTConnect.__init__)
    assert list(sig.parameters) == ["self", "start", "goal", "env", "max_dist", "sample_num", "goal_sample_rate"]
    assert [sig.parameters[k].default for k in ("max_dist", "sample_num", "goal_sample_rate")] == [0.5, 10000, 0.05]
    assert callable(pmp.RRTConnect.plan_batch)


def test_factory_name_stays_out():
    """The factory keeps refusing the name (test_informed_rrt_fixture.py pins it): construct the class."""
    import python_motion_planning_amd as pmp

    with pytest.raises(NotImplementedError):
        pmp.SearchFactory()("rrt_connect", start=(18, 8), goal=(37, 18), env=C.env_of("readme"))


def test_signature_registered_and_symbol_built():
    from python_motion_planning_amd import _lib

    assert "pmp_rrt_connect_batch" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["pmp_rrt_connect_batch"][1]) == 29
    L = _lib.load_library()
    assert hasattr(L, "pmp_rrt_connect_batch") and hasattr(L, "pmp_rrt_connect_lds_nodes")
    assert callable(batch.rrt_connect_batch) and batch.RRT_CONNECT_DEFAULT_CAP == 2048
    assert L.pmp_rrt_connect_lds_nodes() == LDS_NODES


def test_plan_needs_a_device(monkeypatch):
    """Without a HIP device plan() raises and leaves the global generator untouched."""
    import torch

    import python_motion_planning_amd as pmp
    from python_motion_planning_amd._lib import PMPError

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    np.random.seed(5)
    state = np.random.get_state()
    with pytest.raises(PMPError):
        pmp.RRTConnect((18, 8), (37, 18), C.env_of("readme")).plan()
    assert np.array_equal(np.random.get_state()[1], state[1]) and np.random.get_state()[2] == state[2]
