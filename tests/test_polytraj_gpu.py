"""PolynomialTrajectory3D on gfx950 (pmp_polytraj3d_batch) against the reference's own runs
(tests/golden/polytraj.npz, make_golden_polytraj.py), under the rules of polytraj_checks.py."""
import numpy as np
import pytest

import polytraj_checks as C
from golden_io import seg

pytestmark = pytest.mark.gpu

CASES = list(C.cases())
NAMES = [c[1] for c in CASES]


def _prm(vmax, amax, dt):
    from python_motion_planning_amd import _lib

    return _lib.PolyTrajParams.make(vmax, amax, dt)


def _one(r, q=0):
    n = int(r["n_points"][q])
    return r["points"][q, :n].cpu().numpy()


def _same(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


@pytest.mark.parametrize("name", NAMES)
def test_kernel_against_reference_runs(name):
    """Counts exact (402 points for the axis-aligned case); times and segment_times bit-equal for integer
    waypoints; rows within 1e-9 of max(1, |ref|); NaN pattern exact; evaluate(t) at the fixture's times."""
    from python_motion_planning_amd import batch

    i, _, path, p, bc, z = CASES[NAMES.index(name)]
    bcs = None if bc is None else bc[None]
    r = batch.polytraj3d_batch([path], _prm(*p), bc=bcs)
    assert int(r["status"][0]) == 0
    exact = C.compare_case(z, i, path, _one(r), float(r["total_time"][0]),
                           r["segment_times"][: len(path) - 1].cpu().numpy())
    print(f"{name}: {int(r['n_points'][0])} points, bit-exact {exact}")
    et = seg(z["eval_t"], z["eval_off"], i)
    e = batch.polytraj3d_batch([path], _prm(*p), bc=bcs, eval_t=et)
    assert int(e["status"][0]) == 0 and int(e["n_points"][0]) == len(et)
    C.close(_one(e), seg(z["eval_pts"], z["eval_off"], i), f"{name} evaluate")


def test_batch_equals_single_runs():
    """All fixture paths of one parameter set in one launch give the per-path results bit for bit."""
    from python_motion_planning_amd import batch

    sel = [c for c in CASES if c[3] == CASES[NAMES.index("d_diag")][3]]
    assert len(sel) >= 4
    bc = np.stack([np.zeros((4, 3)) if c[4] is None else c[4] for c in sel])
    r = batch.polytraj3d_batch([c[2] for c in sel], _prm(*sel[0][3]), bc=bc)
    so = r["seg_off"]
    for j, c in enumerate(sel):
        s = batch.polytraj3d_batch([c[2]], _prm(*c[3]), bc=bc[j][None])
        assert int(r["n_points"][j]) == int(s["n_points"][0]) and int(r["status"][j]) == 0
        assert _same(_one(r, j), _one(s)), c[1]
        assert float(r["total_time"][j]) == float(s["total_time"][0])
        n = len(c[2])
        assert np.array_equal(r["segment_times"][so[j]:so[j] + n - 1].cpu().numpy(), s["segment_times"][: n - 1].cpu().numpy())


def test_cells_form_equals_host_decoded():
    """64 A* 3D paths left on the device, decoded in the kernel, against the same paths decoded on the host."""
    from python_motion_planning_amd import batch, workloads as wl

    occ, s, g = wl.c5_workload(64)
    a = batch.astar3d_batch(occ, s, g, path_cap=256)
    X, Y, Z = occ.shape[-3:]
    pl, P = a["path_len"].cpu().numpy(), a["path"].cpu().numpy()
    assert (pl >= 2).sum() >= 48 and pl.max() <= 256
    paths = []
    for q in range(len(pl)):
        v = P[q, : pl[q]].astype(np.int64)
        paths.append(np.stack([v // (Y * Z), (v // Z) % Y, v % Z], axis=1).astype(np.float64))
    prm = _prm((2.0, 2.0, 1.5), (1.5, 1.5, 1.0), 0.05)
    h = batch.polytraj3d_batch(paths, prm)
    c = batch.polytraj3d_batch(None, prm, cells=(a["path"], a["path_len"], (X, Y, Z)))
    assert np.array_equal(h["status"].cpu().numpy(), c["status"].cpu().numpy())
    assert set(h["status"].cpu().numpy().tolist()) <= {0, 4} and (h["status"].cpu().numpy() == 0).sum() >= 48
    assert np.array_equal(h["n_points"].cpu().numpy(), c["n_points"].cpu().numpy())
    assert np.array_equal(h["total_time"].cpu().numpy(), c["total_time"].cpu().numpy())
    hp, cp = h["points"].cpu().numpy(), c["points"].cpu().numpy()
    for q in range(len(pl)):
        n = int(h["n_points"][q])
        assert _same(hp[q, :n], cp[q, :n]), q
        assert np.array_equal(h["segment_times"][h["seg_off"][q]:h["seg_off"][q] + max(pl[q] - 1, 0)].cpu().numpy(),
                              c["segment_times"][q, : max(pl[q] - 1, 0)].cpu().numpy())


def test_resample():
    from python_motion_planning_amd import batch

    z = CASES[0][5]
    i, _, path, p, bc, _ = CASES[int(z["rs_case"])]
    r = batch.polytraj3d_batch([path], _prm(*p), sample_dt=float(z["rs_dt"]))
    rows = _one(r)
    assert len(rows) == len(z["rs_pts"]) and np.array_equal(rows[:, 0], z["rs_pts"][:, 0])
    C.close(rows, z["rs_pts"], "resample")


def test_dropin_polynomial_trajectory():
    """The drop-in class as examples/3d_example.py:104-137 uses it: optimize_time_allocation(5), generate(),
    check_constraints(); then evaluate() and resample()."""
    from python_motion_planning_amd import PolynomialTrajectory3D, TrajectoryConstraints

    z = CASES[0][5]
    for name in ("b_two", "d_diag"):
        i, _, path, (vmax, amax, dt), bc, _ = CASES[NAMES.index(name)]
        mj = z["max_jerk"][i]
        cons = TrajectoryConstraints(max_velocity=np.array(vmax), max_acceleration=np.array(amax),
                                     max_jerk=None if np.isnan(mj).any() else mj, min_time_step=dt)
        tr = PolynomialTrajectory3D(path=[tuple(v) for v in path], constraints=cons)
        tr.optimize_time_allocation(max_iterations=5)
        C.times_match(tr.segment_times, seg(z["opt_seg_times"], z["seg_off"], i), False, f"{name} scaled times")
        C.times_match([tr.total_time], [z["opt_total"][i]], False, f"{name} scaled total")
        assert len(tr.trajectory_points) == int(z["opt_n"][i])
        if name == "b_two":
            assert tr.total_time > z["total_time"][i]
        pts = tr.generate()
        assert tr.total_time == z["regen_total"][i] and len(pts) == int(z["regen_n"][i])
        assert np.array_equal(tr.segment_times, seg(z["seg_times"], z["seg_off"], i))
        rows = np.array([[q.time, *q.position, *q.velocity, *q.acceleration, *q.jerk,
                          np.nan if q.yaw is None else q.yaw, np.nan if q.yaw_rate is None else q.yaw_rate] for q in pts])
        C.close(rows, seg(z["pts"], z["pts_off"], i), f"{name} class rows")
        cs = tr.check_constraints()
        assert [cs["velocity_satisfied"], cs["acceleration_satisfied"], cs["jerk_satisfied"]] == z["checks"][i].tolist()
        e = tr.evaluate(pts[3].time)
        assert np.array_equal(e.velocity, pts[3].velocity) and np.array_equal(e.jerk, pts[3].jerk) and e.yaw is None
        assert tr.evaluate(-1.0).time == 0.0 and tr.evaluate(tr.total_time + 5).time == tr.total_time
        assert tr.get_positions().shape == (len(pts), 3) and tr.get_times()[-1] == tr.total_time
        if name == "d_diag":
            rs = tr.resample(float(z["rs_dt"]))
            assert [q.time for q in rs] == z["rs_pts"][:, 0].tolist() and rs[5].yaw is None
            C.close(np.array([q.position for q in rs]), z["rs_pts"][:, 1:4], "class resample")
    # a trajectory that was never generated: evaluate() generates first
    tr = PolynomialTrajectory3D([(0, 0, 0), (1, 0, 0), (2, 0, 0)])
    assert np.allclose(tr.evaluate(4.0).position, [2.0, 0.0, 0.0], rtol=0, atol=1e-12) and len(tr.trajectory_points) == 402


def test_statuses():
    """2 (point_cap too small: the count is reported, and the retry delivers the rows), 3 (more waypoints
    than max_waypoints), 4 (fewer than two waypoints)."""
    from python_motion_planning_amd import _lib, batch

    i, _, path, p, bc, z = CASES[NAMES.index("i_long")]
    n = int(z["n_pts"][i])
    r = batch.polytraj3d_batch([path], _prm(*p), point_cap=100, retry_overflow=False)
    assert int(r["status"][0]) == 2 and int(r["n_points"][0]) == n and r["points"].shape[1] == 100
    full = batch.polytraj3d_batch([path], _prm(*p))
    assert np.array_equal(r["points"][0].cpu().numpy(), full["points"][0, :100].cpu().numpy(), equal_nan=True)
    short = np.array([[0.0, 0, 0], [1, 0, 0]])
    r = batch.polytraj3d_batch([short, path], _prm(*p), point_cap=100)
    assert r["status"].cpu().numpy().tolist() == [0, 0] and r["n_points"].cpu().numpy().tolist()[1] == n
    assert r["points"].shape[1] >= n
    C.compare_case(z, i, path, _one(r, 1), float(r["total_time"][1]), r["segment_times"][2:2 + len(path) - 1].cpu().numpy())
    limit = _lib.load_library().pmp_polytraj3d_max_waypoints()
    assert limit >= 480
    long_path = np.column_stack([np.arange(limit + 1), np.zeros(limit + 1), np.zeros(limit + 1)]).astype(np.float64)
    r = batch.polytraj3d_batch([long_path[:5], long_path, np.array([[1.0, 1.0, 1.0]]), np.zeros((0, 3))], _prm(*p), point_cap=64)
    assert r["status"].cpu().numpy().tolist() == [0, 3, 4, 4]
    r = batch.polytraj3d_batch([long_path[:5], long_path[:4]], _prm(*p), max_waypoints=4, point_cap=64, retry_overflow=False)
    assert r["status"].cpu().numpy().tolist() == [3, 2]


def test_full_waypoint_cap():
    """A path of exactly the largest max_waypoints (the whole LDS block) against the sequential restatement."""
    from python_motion_planning_amd import _lib, batch

    limit = _lib.load_library().pmp_polytraj3d_max_waypoints()
    rng = np.random.default_rng(3)
    path = (np.cumsum(rng.integers(-1, 2, size=(limit, 3)), axis=0) + 100).astype(np.float64)
    prm = ((2.0, 2.0, 1.5), (1.5, 1.5, 1.0), 0.5)
    r = batch.polytraj3d_batch([path], _prm(*prm))
    o = C.restate(path, *prm)
    assert int(r["status"][0]) == 0 and float(r["total_time"][0]) == o["total_time"]
    assert np.array_equal(r["segment_times"][: limit - 1].cpu().numpy(), o["segment_times"])
    rows = _one(r)
    assert np.array_equal(rows[:, 0], o["points"][:, 0])
    C.close(rows, o["points"], "full cap")


def test_refused_constraints():
    """PMP_EINVAL where the reference divides by zero or never leaves its sampling loop"""
    from python_motion_planning_amd import _lib, batch

    path = [np.array([[0.0, 0, 0], [1, 0, 0]])]
    for vmax, amax, dt in (((2.0,) * 3, (1.0, 0.0, 1.0), 0.01), ((2.0,) * 3, (1.0, -1.0, 1.0), 0.01),
                           ((2.0, np.inf, 2.0), (1.0,) * 3, 0.01), ((2.0,) * 3, (1.0, np.nan, 1.0), 0.01),
                           ((2.0,) * 3, (1.0,) * 3, 0.0), ((2.0,) * 3, (1.0,) * 3, -0.01), ((2.0,) * 3, (1.0,) * 3, np.inf)):
        with pytest.raises(_lib.PMPError, match="pmp_polytraj3d_batch"):
            batch.polytraj3d_batch(path, _prm(vmax, amax, dt), point_cap=64)
