"""HIP PID / APF / RPP (follow.hip via the C-ABI) vs the reference's runs (tests/golden/follow_plans.npz)
and, for batches the reference cannot produce, the sequential restatement (follow_checks.run).

Bars: step counts, statuses and return conventions equal; poses, lookahead points, the robot's final
state and PID's integrators within rtol = atol = 1e-9 (device atan2 / sin / cos <= 1 ulp from glibc;
the reference's own runs keep their step counts and stay within 1e-11 under such noise, see
make_golden_follow.py)."""
import numpy as np
import pytest

import follow_checks as fc

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-9, atol=1e-9)
CASES = list(fc.cases())


def _lp(kind):
    from python_motion_planning_amd import _lib

    return _lib.LPParams.from_params(fc.lp_params(kind))


def _fp(**over):
    from python_motion_planning_amd import _lib

    return _lib.FollowParams.make(**over)


@pytest.fixture(scope="module")
def env():
    return fc.readme_env()


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_plan_dropin_against_reference(c, env):
    import python_motion_planning_amd as pmp

    kind = c["kind"]
    cls = {"pid": pmp.PID, "apf": pmp.APF, "rpp": pmp.RPP}[kind]
    params = {} if c["max_iteration"] == 1500 else dict(MAX_ITERATION=c["max_iteration"])
    planner = cls(tuple(c["start"]), tuple(c["goal"]), env, **params)
    assert str(planner) == str(c["str"])
    assert np.array_equal(np.asarray(planner.path, np.float64), c["path"])
    if kind == "rpp":
        planner.scaling_dist = c["over"]["scaling_dist"]  # attributes are read at each call
        planner.regulated_radius_min = c["over"]["regulated_radius_min"]
    if c["exc"]:
        with pytest.raises(ZeroDivisionError):
            planner.plan()
    else:
        ret = planner.plan()
        if bool(c["ok"]):
            assert ret[0] is True and ret[1] is planner.robot.history_pose and len(ret) == (3 if kind == "rpp" else 2)
            if kind == "rpp":
                assert len(ret[2]) == len(c["look"])
                np.testing.assert_allclose(np.array(ret[2]).reshape(-1, 2), c["look"], **TOL)
        else:
            assert ret == ((False, None, None) if kind == "rpp" else (False, None))
    r = planner.robot
    assert len(r.history_pose) == len(c["poses"])
    np.testing.assert_allclose(np.array(r.history_pose).reshape(-1, 3), c["poses"], **TOL)
    np.testing.assert_allclose([r.px, r.py, r.theta, r.v, r.w], c["final"], **TOL)
    if kind == "pid":
        np.testing.assert_allclose([planner.e_v, planner.i_v, planner.e_w, planner.i_w], c["integrators"], **TOL)


def _c4(na):
    """C4 agents with their A* paths; agent 1 stands at its goal (reachGoal holds: 0 steps)."""
    from python_motion_planning_amd import batch, workloads as wl

    occ, states, goals = wl.c4_workload(na)
    states[1] = [45.0, 25.0, 0.1, 0.0, 0.0]
    r = batch.astar2d_batch(occ, states[:, :2].astype(np.int32), np.tile([45, 25], (na, 1)).astype(np.int32),
                            path_cap=2048)
    pl, P, H = r["path_len"].cpu().numpy(), r["path"].cpu().numpy(), occ.shape[1]
    paths = [np.column_stack([P[i, : pl[i]][::-1] // H, P[i, : pl[i]][::-1] % H]).astype(np.float64)
             for i in range(na)]
    return occ, states, goals, paths


def _launch(kind, grid, states, goals, paths, iters, fp=None, pid=None, **kw):
    import torch

    from python_motion_planning_amd import batch

    xy, off = batch.pack_paths(paths)
    st = torch.tensor(states, dtype=torch.float64, device="cuda")
    pd = torch.tensor(np.zeros((len(states), 4)) if pid is None else pid, dtype=torch.float64, device="cuda")
    out = batch.follow_step_batch(kind, grid, _lp(kind), fp or _fp(), st, goals, xy, off, iters=iters, pid_state=pd, **kw)
    return out, st, pd


@pytest.mark.parametrize("kind", fc.KINDS)
def test_c4_batch_against_restatement(kind):
    """37 agents (not a multiple of the four rows of a wave), 40 iterations; one agent finishes at once."""
    na, iters = 37, 40
    occ, states, goals, paths = _c4(na)
    grid = (0, 0, occ.astype(np.uint8))
    out, st, pd = _launch(kind, grid, states, goals, paths, iters, want_hist=True, want_lookahead=True)
    ref = [fc.run(kind, paths[i], goals[i], states[i], iters, grid=grid) for i in range(na)]
    n = out["n_steps"].cpu().numpy()
    assert np.array_equal(out["status"].cpu().numpy(), [r["status"] for r in ref])
    assert np.array_equal(n, [r["n_steps"] for r in ref])
    assert n[1] == 0 and int(out["status"][1]) == fc.REACHED and n[0] > 0 and n[2] > 0 and n[3] > 0
    np.testing.assert_allclose(st.cpu().numpy(), np.array([r["state"] for r in ref]), **TOL)
    if kind == "pid":
        np.testing.assert_allclose(pd.cpu().numpy(), np.array([r["pid"] for r in ref]), **TOL)
    hp, lk = out["hist_pose"].cpu().numpy(), out["lookahead"].cpu().numpy()
    for i in range(na):
        np.testing.assert_allclose(hp[i, : n[i]], ref[i]["poses"], **TOL)
        np.testing.assert_allclose(lk[i, : n[i]], ref[i]["look"], **TOL)
    moved = sum(int(r["n_steps"] - r["counters"][0] - r["counters"][1]) for r in ref)
    assert moved > na  # the controllers proper ran, not only the rotate branches


@pytest.mark.parametrize("kind", ["apf", "rpp"])
def test_window_at_grid_edges_against_all_obstacle_cells(kind):
    """One step for agents near two corners of the grid's box and left of it (a negative coordinate),
    d_0 = scaling_dist = 2.5, headed so that the obstacle term decides the control; the expected value
    takes the sum / minimum over all obstacle cells."""
    grid = fc.readme_grid()
    c = next(c for c in CASES if c["name"] == "reach_a" and c["kind"] == kind)
    f = fc.follow_params(scaling_dist=2.5, d_0=2.5)
    pos = [(1.2, 1.3), (49.6, 29.5), (-0.4, 15.2)]
    states = []
    for x, y in pos:
        tr = []
        fc.run(kind, c["path"], c["goal"], [x, y, 0.0, 0.0, 0.0], 1, f=f, grid=grid, brute=True, trace=tr)
        states.append([x, y, tr[0]["theta_d"] + 0.05, 0.0, 0.0])  # v = 0: theta_d does not depend on theta
    states = np.array(states)
    goals = np.tile(c["goal"], (3, 1))
    paths = [c["path"]] * 3
    ref, trs = [], []
    for s in states:
        tr = []
        ref.append(fc.run(kind, c["path"], c["goal"], s, 1, f=f, grid=grid, brute=True, trace=tr))
        trs.append(tr[0])
    for r, tr in zip(ref, trs):  # the term is in force, and the control is not saturated by it
        assert r["n_steps"] == 1 and r["counters"][0] == 0 and r["counters"][1] == 0
        if kind == "apf":
            assert tr["rep"] != (0.0, 0.0) and abs(r["state"][4]) < 1.0
        else:
            assert tr["dmin"] < 2.5 and r["counters"][4] == 1 and 0 < r["state"][3] < 0.5
    out, st, _ = _launch(kind, grid, states, goals, paths, 1, fp=_fp(scaling_dist=2.5, d_0=2.5))
    assert np.array_equal(out["n_steps"].cpu().numpy(), [1, 1, 1])
    np.testing.assert_allclose(st.cpu().numpy(), np.array([r["state"] for r in ref]), **TOL)


@pytest.mark.parametrize("kind", fc.KINDS)
def test_single_iteration_calls_carry_state(kind):
    """50 calls of one iteration equal one call of 50, bit for bit (state and PID's integrators carry)."""
    import torch

    from python_motion_planning_amd import batch

    na = 7
    occ, states, goals, paths = _c4(na)
    grid = (0, 0, occ.astype(np.uint8))
    out, st, pd = _launch(kind, grid, states, goals, paths, 50)
    xy, off = batch.pack_paths(paths)
    st1 = torch.tensor(states, dtype=torch.float64, device="cuda")
    pd1 = torch.zeros((na, 4), dtype=torch.float64, device="cuda")
    steps = np.zeros(na, np.int64)
    for _ in range(50):
        o = batch.follow_step_batch(kind, grid, _lp(kind), _fp(), st1, goals, xy, off, iters=1, pid_state=pd1)
        steps += o["n_steps"].cpu().numpy()
    assert np.array_equal(st1.cpu().numpy(), st.cpu().numpy())
    assert np.array_equal(pd1.cpu().numpy(), pd.cpu().numpy())
    assert np.array_equal(steps, out["n_steps"].cpu().numpy())
    assert np.array_equal(o["status"].cpu().numpy(), out["status"].cpu().numpy())
    if kind == "pid":
        assert np.abs(pd.cpu().numpy()).max() > 0


def test_empty_obstacle_set_raises_value_error():
    import python_motion_planning_amd as pmp

    env = fc.readme_env()
    for cls in (pmp.APF, pmp.RPP):
        planner = cls((5, 5, 0), (45, 25, 0), env)
        planner.obstacles = set()
        with pytest.raises(ValueError):
            planner.plan()


def test_factory_names_still_raise():
    import python_motion_planning_amd as pmp

    for name in ("pid", "apf", "rpp"):
        with pytest.raises(NotImplementedError):
            pmp.ControlFactory()(name, start=(5, 5, 0), goal=(45, 25, 0), env=None)
