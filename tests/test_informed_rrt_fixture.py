"""Informed RRT* without a device: the fixture of reference runs is what the issue asks for, the
sequential restatement of the kernel's arithmetic (informed_rrt_checks.plan) reproduces every one of
its cases bit for bit, and the feature is exposed through every layer."""
import inspect

import numpy as np
import pytest

import informed_rrt_checks as C

CASES, Z = C.cases()


def test_fixture_covers_the_cases():
    assert int(Z["n_tree"]) == 16 and int(Z["n_scanned"]) == 200
    plain = CASES[: int(Z["n_tree"])]
    assert [(c["map"], c["seed"], c["sample_num"]) for c in plain] == (
        [("readme", s, 1500) for s in range(12)] + [("readme", 0, 400), ("readme", 1, 400)]
        + [("c3", 2, 3000), ("c3", 3, 3000)])
    assert sum(len(c["finds"]) >= 2 for c in CASES) >= 8
    assert sum(len(c["finds"]) == 0 and not c["cycle"] for c in CASES) >= 2
    assert sum(c["draws"] > 3 * c["sample_num"] + 1 for c in CASES) >= 2
    assert len(CASES) - len(plain) <= 2 and all(c["cycle"] for c in CASES[len(plain):])
    c0 = CASES[0]
    assert (c0["best_cost"], c0["n_nodes"]) == (26.33608540485134, 1032)
    assert [CASES[14]["draws"], CASES[15]["draws"]] == [9525, 9424]
    # InformedRRT(..., goal_sample_rate=0.3) planned exactly like the default (the constructor drops it)
    assert np.array_equal(Z["quirk_summary"], np.array([c0["n_nodes"], c0["goal_slot"], len(c0["finds"]),
                                                        c0["best_cost"], c0["next"], c0["draws"]], np.float64))
    for c in CASES:
        assert c["best_cost"] == (c["finds"].min() if len(c["finds"]) else np.inf)
        assert (c["goal_slot"] >= 0) == (len(c["finds"]) > 0 or c["cycle"])
        assert C.stream(c)[c["draws"]] == c["next"]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_restatement_reproduces_reference(i):
    """Tree, parents, goal slot, the cost at every find, best path, draw count: equal, not close."""
    c = CASES[i]
    rnd = C.stream(c, 4 * c["sample_num"] + 64)
    r = C.plan(c["map"], c["start"], c["goal"], rnd.tolist(), c["sample_num"], max_dist=c["max_dist"], radius=c["r"])
    assert r["status"] == (C.REF_RAISES if c["cycle"] else C.FOUND if len(c["finds"]) else C.NO_PATH)
    assert len(r["x"]) == c["n_nodes"]
    assert np.array_equal(np.array(r["parent"], np.int32), c["parent"])
    assert np.array_equal(np.column_stack([r["x"], r["y"], r["g"]]), c["tree"])
    assert r["goal_slot"] == c["goal_slot"]
    assert np.array_equal(np.array(r["finds"], np.float64), c["finds"])
    assert r["best_cost"] == c["best_cost"]
    assert r["draws"] == c["draws"] and rnd[r["draws"]] == c["next"]
    if len(c["finds"]) and not c["cycle"]:
        assert np.array_equal(np.array(r["best_path"], np.float64), c["path"])
        assert tuple(c["path"][0]) == tuple(c["goal"]) and tuple(c["path"][-1]) == tuple(c["start"])


def test_restatement_stream_overflow():
    """A C3 case with the 3n+1 stream of RRT*: the rejection sampler runs out of draws."""
    c = CASES[14]
    n = 3 * c["sample_num"] + 1
    assert c["draws"] > n
    # (only up to the overflow: the tree is the reference's up to that draw)
    r = C.plan(c["map"], c["start"], c["goal"], C.stream(c, n).tolist(), c["sample_num"], max_dist=c["max_dist"],
               radius=c["r"])
    assert r["status"] == C.CAP_OVERFLOW and n - 1 <= r["draws"] <= n


# ---- exposure: each of these fails without the feature --------------------------------------------------
def test_exported_and_subclass():
    import python_motion_planning_amd as pmp

    assert "InformedRRT" in pmp.__all__
    assert issubclass(pmp.InformedRRT, pmp.RRTStar)
    p = pmp.InformedRRT((18, 8), (37, 18), C.env_of("readme"))
    assert str(p) == "Informed RRT*" and (p.sample_num, p.r, p.max_dist) == (1500, 12.0, 0.5)
    assert p.c_best == float("inf") and p.c_min == float(np.hypot(19, 10))
    sig = inspect.signature(pmp.InformedRRT.__init__)
    assert list(sig.parameters) == ["self", "start", "goal", "env", "max_dist", "sample_num", "r", "goal_sample_rate"]


def test_goal_sample_rate_is_dropped():
    import python_motion_planning_amd as pmp

    p = pmp.InformedRRT((18, 8), (37, 18), C.env_of("readme"), goal_sample_rate=0.3)
    assert p.goal_sample_rate == 0.05 and p.r == 12.0


def test_factory_names():
    import python_motion_planning_amd as pmp

    p = pmp.SearchFactory()("informed_rrt", start=(18, 8), goal=(37, 18), env=C.env_of("readme"))
    assert type(p) is pmp.InformedRRT
    with pytest.raises(NotImplementedError):
        pmp.SearchFactory()("rrt_connect", start=(18, 8), goal=(37, 18), env=C.env_of("readme"))


def test_signature_registered_and_batch_callable():
    from python_motion_planning_amd import _lib, batch

    assert "pmp_informed_rrt_batch" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["pmp_informed_rrt_batch"][1]) == 29
    assert hasattr(_lib.load_library(), "pmp_informed_rrt_batch")
    assert callable(batch.informed_rrt_batch)
    # the host-side ellipse constants are the restatement's (the reference's numpy expressions)
    e = batch.ellipse_constants([(18, 8), (5, 5)], [(37, 18), (505, 505)])
    assert np.array_equal(e, np.array([C.ellipse_constants((18.0, 8.0), (37.0, 18.0)),
                                       C.ellipse_constants((5.0, 5.0), (505.0, 505.0))]))


def _no_gpu():
    import torch

    return not torch.cuda.is_available()


@pytest.mark.skipif(not _no_gpu(), reason="checks the behaviour on a host without a HIP device")
def test_plan_needs_a_device():
    import python_motion_planning_amd as pmp
    from python_motion_planning_amd._lib import PMPError

    state = np.random.get_state()
    with pytest.raises(PMPError):
        pmp.InformedRRT((18, 8), (37, 18), C.env_of("readme")).plan()
    assert np.array_equal(np.random.get_state()[1], state[1])
