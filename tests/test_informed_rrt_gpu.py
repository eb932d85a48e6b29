"""HIP Informed RRT* (rrt.hip's informed mode via pmp_informed_rrt_batch) vs the reference's runs
(tests/golden/informed_rrt.npz) and the sequential restatement (informed_rrt_checks.py).

Bar, as for RRT / RRT* (test_rrt_gpu.py): node count, every parent index, the goal's slot, the number
of connections, the status and the draw count equal; coordinates, costs, the best cost and the best
path within 1e-12 relative (the device atan2 / cos / sin are <= 1 ulp from glibc, which steering
feeds into the node coordinates)."""
import numpy as np
import pytest

import informed_rrt_checks as C

pytestmark = pytest.mark.gpu

RTOL = 1e-12


def _expected_status(c):
    return C.REF_RAISES if c["cycle"] else C.FOUND if len(c["finds"]) else C.NO_PATH


def _check_case(out, q, c, rnd, what):
    n = int(out["n_nodes"][q])
    assert n == c["n_nodes"], (what, n, c["n_nodes"])
    xy = out["tree_xy"][q, :n].cpu().numpy()
    g = out["tree_g"][q, :n].cpu().numpy()
    par = out["tree_parent"][q, :n].cpu().numpy()
    assert np.array_equal(par, c["parent"]), what
    assert int(out["goal_slot"][q]) == c["goal_slot"], what
    assert int(out["n_finds"][q]) == len(c["finds"]), what
    assert int(out["status"][q]) == _expected_status(c), what
    assert rnd[int(out["draws"][q])] == c["next"] and int(out["draws"][q]) == c["draws"], what
    np.testing.assert_allclose(xy, c["tree"][:, :2], rtol=RTOL, atol=0, err_msg=str(what))
    np.testing.assert_allclose(g, c["tree"][:, 2], rtol=RTOL, atol=0, err_msg=str(what))
    best = float(out["best_cost"][q])
    if len(c["finds"]):
        assert abs(best - c["best_cost"]) <= RTOL * c["best_cost"], what
    else:
        assert best == np.inf and int(out["path_len"][q]) == 0, what
    if len(c["finds"]) and not c["cycle"]:
        plen = int(out["path_len"][q])
        assert plen == len(c["path"]), what
        np.testing.assert_allclose(out["path"][q, :plen].cpu().numpy(), c["path"], rtol=RTOL, atol=0, err_msg=str(what))
    return bool(np.array_equal(xy, c["tree"][:, :2]) and np.array_equal(g, c["tree"][:, 2]))


def test_fixture_cases_against_reference():
    """Every fixture case (README finds, never-found, C3 with draws > 3n+1, the parent-cycle run),
    batched per map and setting."""
    from python_motion_planning_amd import batch

    cases, _ = C.cases()
    groups = {}
    for i, c in enumerate(cases):
        groups.setdefault((c["map"], c["sample_num"], c["max_dist"], c["r"], tuple(c["goal"])), []).append(i)
    assert len(groups) == 3
    exact = 0
    for (mp, sn, md, r, _), idx in groups.items():
        rnd = np.stack([C.stream(cases[i], 4 * sn + 64) for i in idx])
        out = batch.informed_rrt_batch(C.env_of(mp), [cases[i]["start"] for i in idx], [cases[i]["goal"] for i in idx],
                                       rnd, sn, max_dist=md, radius=r)
        for q, i in enumerate(idx):
            exact += _check_case(out, q, cases[i], rnd[q], (mp, cases[i]["seed"], sn))
    print(f"{exact}/{len(cases)} trees bit-exact")


def test_dropin_readme():
    """np.random.seed(0); InformedRRT((18, 8), (37, 18), README map).plan(): the reference's cost, path
    and node count, the global generator left where the reference leaves it, c_best set."""
    import python_motion_planning_amd as pmp

    cases, _ = C.cases()
    c = cases[0]
    assert (c["map"], c["seed"], c["sample_num"]) == ("readme", 0, 1500)
    planner = pmp.InformedRRT((18, 8), (37, 18), C.env_of("readme"))
    np.random.seed(0)
    cost, path, expand = planner.plan()
    assert np.random.random() == c["next"]
    assert abs(cost - 26.33608540485134) <= RTOL * cost and planner.c_best == cost
    assert len(expand) == 1032 and len(path) == len(c["path"])
    np.testing.assert_allclose(np.array(path, np.float64), c["path"], rtol=RTOL)
    assert path[0] == (37, 18) and path[-1] == (18, 8)
    assert expand[0] is planner.start and expand[c["goal_slot"]] is planner.goal
    # the goal carries its final parent and g, not the best connection's
    gp = expand[c["parent"][c["goal_slot"]]]
    assert planner.goal.parent == gp.current
    assert abs(planner.goal.g - c["tree"][c["goal_slot"], 2]) <= RTOL * planner.goal.g


def test_never_found_returns_inf_none():
    import python_motion_planning_amd as pmp

    cases, _ = C.cases()
    c = cases[12]
    assert len(c["finds"]) == 0 and c["sample_num"] == 400
    planner = pmp.InformedRRT((18, 8), (27, 13), C.env_of("readme"), sample_num=400)
    np.random.seed(c["seed"])
    cost, path, expand = planner.plan()
    assert cost == float("inf") and path is None and len(expand) == c["n_nodes"]
    assert planner.c_best == float("inf")
    assert np.random.random() == c["next"]


def test_goal_sample_rate_quirk():
    """InformedRRT(..., goal_sample_rate=0.3) plans exactly like the default (informed_rrt.py:61)."""
    import python_motion_planning_amd as pmp

    cases, z = C.cases()
    c = cases[0]
    planner = pmp.InformedRRT((18, 8), (37, 18), C.env_of("readme"), goal_sample_rate=0.3)
    np.random.seed(0)
    cost, path, expand = planner.plan()
    nxt = np.random.random()
    q = z["quirk_summary"]
    assert (len(expand), [n.current for n in expand].index((37, 18)), nxt) == (int(q[0]), int(q[1]), q[4])
    assert abs(cost - q[3]) <= RTOL * q[3] and len(path) == len(c["path"])


def test_stream_overflow_and_rerun(monkeypatch):
    """A C3 case with RRT*'s 3n+1 stream runs out of draws in the rejection sampler (status 3); plan()
    doubles its stream and re-runs -- on the wall query (informed_rrt_checks.WALL_QUERY), whose 5063
    draws exceed the 4n+64 plan() starts with, the result is the restatement's."""
    import python_motion_planning_amd as pmp
    from python_motion_planning_amd import batch

    cases, _ = C.cases()
    c = cases[14]
    sn = c["sample_num"]
    assert c["map"] == "c3" and c["draws"] > 3 * sn + 1
    out = batch.informed_rrt_batch(C.env_of("c3"), [c["start"]], [c["goal"]], C.stream(c, 3 * sn + 1)[None], sn,
                                   max_dist=c["max_dist"], radius=c["r"])
    assert int(out["status"][0]) == C.CAP_OVERFLOW
    assert 3 * sn <= int(out["draws"][0]) <= 3 * sn + 1

    W = C.WALL_QUERY
    sn = W["sample_num"]
    rnd = np.random.RandomState(W["seed"]).random_sample(8 * sn + 128)
    ref = C.plan(C.WALL_MAP, W["start"], W["goal"], rnd.tolist(), sn, max_dist=W["max_dist"])
    assert ref["draws"] == W["draws"] > 4 * sn + 64 and ref["status"] == C.FOUND
    strides = []
    real = batch.informed_rrt_batch

    def spy(env, starts, goals, r, *a, **kw):
        strides.append(r.shape[-1])
        return real(env, starts, goals, r, *a, **kw)

    monkeypatch.setattr(batch, "informed_rrt_batch", spy)
    planner = pmp.InformedRRT(W["start"], W["goal"], C.env_of(C.WALL_MAP), max_dist=W["max_dist"], sample_num=sn)
    np.random.seed(W["seed"])
    cost, path, expand = planner.plan()
    assert strides == [4 * sn + 64, 8 * sn + 128]
    assert np.random.random() == rnd[W["draws"]]
    assert len(expand) == len(ref["x"]) and len(path) == len(ref["best_path"])
    assert abs(cost - ref["best_cost"]) <= RTOL * cost
    np.testing.assert_allclose(np.array(path, np.float64), np.array(ref["best_path"]), rtol=RTOL)


def test_c3_past_the_lds_share_properties():
    """Reference-free, 4 queries x 30,000 samples on C3 (max_dist 8, r 24): trees past the share of the
    coarse copy held in LDS.  Parents reach the start, rewires never raise a cost, the best cost is at
    least the straight line, the best path runs goal -> start over free edges no longer than its cost."""
    from oracle import oracle as O
    from python_motion_planning_amd import batch, workloads as wl

    rects, circs = wl.c3_map()
    nq, sn = 4, 30000
    rnd = np.stack([np.random.RandomState(700 + q).random_sample(8 * sn) for q in range(nq)])
    starts, goals = np.tile([5.0, 5.0], (nq, 1)), np.tile([505.0, 505.0], (nq, 1))
    out = batch.informed_rrt_batch(C.env_of("c3"), starts, goals, rnd, sn, max_dist=8.0, radius=24.0)
    rng = np.random.default_rng(0)
    c_min = float(np.hypot(500.0, 500.0))
    for q in range(nq):
        assert int(out["status"][q]) == C.FOUND and int(out["n_finds"][q]) >= 1
        n = int(out["n_nodes"][q])
        assert n > 16000  # the LDS share holds about 15,500 nodes of a C3 query's coarse copy
        xy = out["tree_xy"][q, :n].cpu().numpy()
        g = out["tree_g"][q, :n].cpu().numpy()
        par = out["tree_parent"][q, :n].cpu().numpy().astype(np.int64)
        assert par[0] == 0 and g[0] == 0
        p = par.copy()
        for _ in range(20):
            p = p[p]
        assert np.all(p == 0)
        edge = np.hypot(xy[:, 0] - xy[par, 0], xy[:, 1] - xy[par, 1])
        assert np.all(g[1:] >= g[par[1:]] + edge[1:] - 1e-9)
        gs = int(out["goal_slot"][q])
        assert tuple(xy[gs]) == (505.0, 505.0)
        best = float(out["best_cost"][q])
        assert c_min <= best < np.inf
        assert int(out["draws"][q]) <= rnd.shape[1]
        plen = int(out["path_len"][q])
        path = out["path"][q, :plen].cpu().numpy()
        assert tuple(path[0]) == (505.0, 505.0) and tuple(path[-1]) == (5.0, 5.0)
        # (a rewire lowers a node's g without touching its descendants': goal.g bounds the length from above)
        seg = np.hypot(*(path[1:] - path[:-1]).T)
        assert c_min <= seg.sum() * (1 + 1e-12) and seg.sum() <= best * (1 + 1e-9)
        for a, b in zip(path[:-1], path[1:]):
            assert not O.map_collision(rects, circs, 512, 512, a, b)
        for j in rng.choice(np.arange(1, n), 200, replace=False):
            assert not O.map_collision(rects, circs, 512, 512, xy[j], xy[par[j]])
