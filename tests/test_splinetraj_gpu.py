"""SplineTrajectory3D on gfx950 (pmp_splinetraj3d_batch) against the reference's own runs
(tests/golden/splinetraj.npz, make_golden_splinetraj.py), under the rules of splinetraj_checks.py."""
import numpy as np
import pytest

import splinetraj_checks as C
from golden_io import seg

pytestmark = pytest.mark.gpu

CASES = list(C.cases())
NAMES = [c[1] for c in CASES]
COLS = ["t", "x", "y", "z", "vx", "vy", "vz", "ax", "ay", "az", "yaw", "yaw_rate"]


def _prm(vmax, amax, dt, degree):
    from python_motion_planning_amd import _lib

    return _lib.SplineTrajParams.make(vmax, amax, dt, degree)


def _one(r, q=0):
    n = int(r["n_points"][q])
    return r["points"][q, :n].cpu().numpy()


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _rows(pts):
    return np.array([[q.time, *q.position, *q.velocity, *q.acceleration, np.nan if q.yaw is None else q.yaw,
                      np.nan if q.yaw_rate is None else q.yaw_rate] for q in pts], np.float64).reshape(-1, 12)


def _groups():
    """the fixture's cases by parameter set (constraints and degree)"""
    g = {}
    for c in CASES:
        g.setdefault((c[3], c[4]), []).append(c)
    return g


@pytest.mark.parametrize("name", NAMES)
def test_class_generate_against_reference_runs(name):
    """The drop-in class per case: count and NaN pattern exact, times and total_time within 1e-12, rows
    within 1e-9 of max(1, |ref|); u_waypoints; check_constraints(); evaluate(t) at the fixture's times."""
    from python_motion_planning_amd import SplineTrajectory3D, TrajectoryConstraints

    i, _, path, (vmax, amax, dt), deg, z = CASES[NAMES.index(name)]
    cons = TrajectoryConstraints(max_velocity=np.array(vmax), max_acceleration=np.array(amax), min_time_step=dt)
    pts_in = [tuple(p[:2]) for p in path] if name == "j_2d" else [tuple(p) for p in path]
    tr = SplineTrajectory3D(path=pts_in, constraints=cons, spline_degree=deg)
    assert tr.spline_degree == int(z["k"][i]) and tr.u_waypoints is None
    e0 = tr.evaluate(float(z["eval_t"][i][2]))  # a fresh object generates first
    assert len(tr.trajectory_points) == int(z["n_pts"][i]) and e0.yaw is None
    rows = _rows(tr.generate())
    err = C.compare_case(z, i, rows, tr.total_time)
    print(f"{name}: {len(rows)} points; largest error per column:", ", ".join(f"{c} {e:.1e}" for c, e in zip(COLS, err)))
    C.times_match(tr.u_waypoints, seg(z["u_waypoints"], z["path_off"], i), f"{name} u_waypoints")
    C.compare_checks(z, i, tr.check_constraints())
    ev = _rows([tr.evaluate(float(t)) for t in z["eval_t"][i]])
    assert np.isnan(ev[:, 10:]).all()
    C.close(ev, z["eval_pts"][i], f"{name} evaluate")
    C.times_match(ev[:, 0], z["eval_pts"][i][:, 0], f"{name} evaluate times")
    assert tr.get_positions().shape == (len(rows), 3) and tr.get_times()[-1] == tr.total_time


def test_batch_equals_single_runs():
    """All fixture paths of one parameter set (mixed lengths) in one launch per degree give the per-path
    results bit for bit."""
    from python_motion_planning_amd import batch

    big = [g for g in _groups().values() if len(g) >= 4]
    assert len(big) >= 2 and {g[0][4] for g in big} >= {3, 5}
    for sel in big:
        prm = _prm(*sel[0][3], sel[0][4])
        r = batch.splinetraj3d_batch([c[2] for c in sel], prm)
        assert len({len(c[2]) for c in sel}) >= 3
        for j, c in enumerate(sel):
            s = batch.splinetraj3d_batch([c[2]], prm)
            assert int(r["status"][j]) == 0 and int(s["status"][0]) == 0
            assert int(r["n_points"][j]) == int(s["n_points"][0]) == int(c[5]["n_pts"][c[0]])
            assert _same(_one(r, j), _one(s)), c[1]
            assert float(r["total_time"][j]) == float(s["total_time"][0])


def test_cells_form_equals_waypoint_form():
    """The integer-waypoint cases as cell ids on a 128 x 128 x 64 grid, decoded in the kernel, against the
    same paths given as waypoints: bit-equal rows."""
    import torch

    from python_motion_planning_amd import batch

    X, Y, Z = 128, 128, 64
    done = 0
    for sel in _groups().values():
        sel = [c for c in sel if np.all(c[2] == np.round(c[2])) and np.all(c[2] >= 0) and np.all(c[2] < [X, Y, Z])]
        if len(sel) < 3:
            continue
        done += len(sel)
        cap = max(len(c[2]) for c in sel) + 3
        cells = np.zeros((len(sel), cap), np.int32)
        for j, c in enumerate(sel):
            p = c[2].astype(np.int64)
            cells[j, : len(p)] = p[:, 0] * Y * Z + p[:, 1] * Z + p[:, 2]
        lens = np.array([len(c[2]) for c in sel], np.int32)
        prm = _prm(*sel[0][3], sel[0][4])
        h = batch.splinetraj3d_batch([c[2] for c in sel], prm)
        k = batch.splinetraj3d_batch(None, prm, cells=(torch.as_tensor(cells, device="cuda"),
                                                       torch.as_tensor(lens, device="cuda"), (X, Y, Z)))
        assert h["status"].cpu().numpy().tolist() == [0] * len(sel) == k["status"].cpu().numpy().tolist()
        assert np.array_equal(h["n_points"].cpu().numpy(), k["n_points"].cpu().numpy())
        assert np.array_equal(h["total_time"].cpu().numpy(), k["total_time"].cpu().numpy())
        for j in range(len(sel)):
            assert _same(_one(h, j), _one(k, j)), sel[j][1]
    assert done >= 8


def test_evaluate_resample_constant_speed():
    """evaluate(t) of every case, resample(0.03) and reparameterize_constant_speed() of the diagonal case"""
    from python_motion_planning_amd import SplineTrajectory3D, TrajectoryConstraints, batch

    z = CASES[0][5]
    for i, name, path, p, deg, _ in CASES:
        e = batch.splinetraj3d_batch([path], _prm(*p, deg), eval_t=z["eval_t"][i])
        assert int(e["status"][0]) == 0 and int(e["n_points"][0]) == 5
        C.close(_one(e), z["eval_pts"][i], f"{name} evaluate")
        C.times_match([float(e["total_time"][0])], [z["total_time"][i]], f"{name} total_time")
    i, name, path, p, deg, _ = CASES[int(z["rs_case"])]
    r = _one(batch.splinetraj3d_batch([path], _prm(*p, deg), sample_dt=float(z["rs_dt"])))
    C.times_match(r[:, 0], z["rs_pts"][:, 0], "resample times")
    C.close(r, z["rs_pts"], "resample")
    c = batch.splinetraj3d_batch([path], _prm(*p, deg), constant_speed=True)
    C.times_match([float(c["total_time"][0])], [z["cs_total"]], "constant-speed total_time")
    C.times_match(_one(c)[:, 0], z["cs_pts"][:, 0], "constant-speed times")
    C.close(_one(c), z["cs_pts"], "constant speed")
    # the class: resample() on the scaled time, then the constant-speed state, then evaluate() on it
    cons = TrajectoryConstraints(max_velocity=np.array(p[0]), max_acceleration=np.array(p[1]), min_time_step=p[2])
    tr = SplineTrajectory3D([tuple(v) for v in path], cons, spline_degree=deg)
    rs = _rows(tr.resample(float(z["rs_dt"])))
    assert _same(rs, r)
    tr.reparameterize_constant_speed()
    assert tr.total_time == float(c["total_time"][0]) and _same(_rows(tr.trajectory_points), _one(c))
    assert all(q.yaw is None for q in tr.trajectory_points)
    mid = tr.evaluate(tr.total_time / 2)
    assert mid.time == tr.total_time / 2
    C.close(mid.position, _one(batch.splinetraj3d_batch([path], _prm(*p, deg), eval_t=[z["total_time"][i] / 2]))[0, 1:4],
            "evaluate after the reparameterisation")


def test_statuses():
    """2 (point_cap too small: the true count is reported, and the retry delivers the rows), 3 (more
    waypoints than max_waypoints), 4 (two waypoints; a repeated waypoint) inside an otherwise good batch,
    whose other rows are unchanged."""
    from python_motion_planning_amd import _lib, batch

    i, name, path, p, deg, z = CASES[NAMES.index("h_diag_k3")]
    prm = _prm(*p, deg)
    n = int(z["n_pts"][i])
    full = batch.splinetraj3d_batch([path], prm)
    r = batch.splinetraj3d_batch([path], prm, point_cap=16, retry_overflow=False)
    assert int(r["status"][0]) == 2 and int(r["n_points"][0]) == n and r["points"].shape[1] == 16
    assert np.array_equal(r["points"][0].cpu().numpy(), full["points"][0, :16].cpu().numpy(), equal_nan=True)
    r = batch.splinetraj3d_batch([path], prm, point_cap=16)
    assert int(r["status"][0]) == 0 and r["points"].shape[1] >= n
    C.compare_case(z, i, _one(r), float(r["total_time"][0]))
    j, _, path5, _, _, _ = CASES[NAMES.index("d_five_k3")]
    two = np.array([[0.0, 0, 0], [1, 2, 0]])
    rep = np.array([[0.0, 0, 0], [1, 2, 0], [1, 2, 0], [3, 3, 1]])
    r = batch.splinetraj3d_batch([path, two, path5, rep, path, np.zeros((0, 3))], prm)
    assert r["status"].cpu().numpy().tolist() == [0, 4, 0, 4, 0, 4]
    assert r["n_points"].cpu().numpy().tolist() == [n, 0, int(z["n_pts"][j]), 0, n, 0]
    assert _same(_one(r, 0), _one(full)) and _same(_one(r, 4), _one(full))
    C.compare_case(z, j, _one(r, 2), float(r["total_time"][2]))
    r = batch.splinetraj3d_batch([path5, path], prm, max_waypoints=5, retry_overflow=False)
    assert r["status"].cpu().numpy().tolist() == [0, 3]
    limit = _lib.load_library().pmp_splinetraj3d_max_waypoints()
    long_path = np.column_stack([np.arange(limit + 1), np.zeros(limit + 1), np.zeros(limit + 1)]).astype(np.float64)
    r = batch.splinetraj3d_batch([path5, long_path], prm, point_cap=64, retry_overflow=False)
    assert r["status"].cpu().numpy().tolist()[1] == 3


def test_full_waypoint_cap():
    """A walk of exactly the largest max_waypoints (the whole LDS block) against the sequential restatement:
    the band solve at its longest."""
    from python_motion_planning_amd import _lib, batch

    limit = _lib.load_library().pmp_splinetraj3d_max_waypoints()
    rng = np.random.default_rng(3)
    step = rng.integers(-1, 2, size=(limit, 3))
    step[:, 0] = 1  # no repeated waypoint
    path = (np.cumsum(step, axis=0) + 100).astype(np.float64)
    prm = ((2.0, 2.0, 1.5), (1.5, 1.5, 1.0), 2.0, 3)
    r = batch.splinetraj3d_batch([path], _prm(*prm))
    o = C.restate(path, *prm)
    assert int(r["status"][0]) == 0
    C.times_match([float(r["total_time"][0])], [o["total_time"]], "full cap total_time")
    rows = _one(r)
    C.times_match(rows[:, 0], o["points"][:, 0], "full cap times")
    C.close(rows, o["points"], "full cap")


def test_refused_parameters():
    """PMP_EINVAL where scipy raises, or the reference divides by zero or never leaves its sampling loop"""
    from python_motion_planning_amd import _lib, batch

    path = [np.array([[0.0, 0, 0], [1, 2, 0], [3, 3, 1]])]
    for vmax, amax, dt, deg in (((2.0,) * 3, (1.0, 0.0, 1.0), 0.01, 3), ((2.0, 0.0, 2.0), (1.0,) * 3, 0.01, 3),
                                ((2.0, np.inf, 2.0), (1.0,) * 3, 0.01, 3), ((2.0,) * 3, (1.0, np.nan, 1.0), 0.01, 3),
                                ((2.0,) * 3, (1.0,) * 3, 0.0, 3), ((2.0,) * 3, (1.0,) * 3, 0.01, 0),
                                ((2.0,) * 3, (1.0,) * 3, 0.01, 6)):
        with pytest.raises(_lib.PMPError, match="pmp_splinetraj3d_batch"):
            batch.splinetraj3d_batch(path, _prm(vmax, amax, dt, deg), point_cap=64)
