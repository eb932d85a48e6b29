"""Generate tests/golden/polytraj.npz by running the REFERENCE's PolynomialTrajectory3D
(trajectory/polynomial_trajectory.py:52-331) with pyvista and osqp stubbed, as make_golden.py does.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_polytraj.py

Per case: the path, the constraints, the boundary conditions, segment_times, total_time, every time
stamp, the rows (time, position, velocity, acceleration, jerk, yaw, yaw rate; NaN = None) -- all of
them for the short cases, the first and last 130 plus every 16th for the long ones (pts_idx) --
check_constraints(), evaluate(t) at times outside the range and on segment ends, resample(0.03) of
the diagonal case, and the state after optimize_time_allocation(5) and after the generate() that
follows it."""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, ragged  # noqa: E402

NAN = float("nan")
EX = ([2.0, 2.0, 1.5], [1.5, 1.5, 1.0], [1.0, 1.0, 0.8], 0.05)  # examples/3d_example.py:104-109


def rows(pts):
    return np.array([[q.time, *q.position, *q.velocity, *q.acceleration, *q.jerk, NAN if q.yaw is None else q.yaw,
                      NAN if q.yaw_rate is None else q.yaw_rate] for q in pts], np.float64).reshape(-1, 15)


def make(path, cons, bc):
    from python_motion_planning.trajectory import PolynomialTrajectory3D, TrajectoryConstraints

    c = None if cons is None else TrajectoryConstraints(max_velocity=np.array(cons[0]), max_acceleration=np.array(cons[1]),
                                                        max_jerk=np.array(cons[2]), min_time_step=cons[3])
    b = None if bc is None else dict(initial_velocity=np.array(bc[0]), final_velocity=np.array(bc[1]),
                                     initial_acceleration=np.array(bc[2]), final_acceleration=np.array(bc[3]))
    return PolynomialTrajectory3D(path=[tuple(p) for p in path], constraints=c, boundary_conditions=b)


def main():
    import_reference()
    rng = np.random.default_rng(7)
    walk = np.cumsum(rng.integers(-1, 2, size=(70, 3)), axis=0) + 40
    bc_f = [[0.3, -0.2, 0.1], [-0.4, 0.25, 0.0], [0.2, 0.1, -0.3], [-0.1, 0.3, 0.2]]
    cases = [  # name, path, constraints (None = defaults), boundary conditions
        ("a_axis3", [(0, 0, 0), (1, 0, 0), (2, 0, 0)], None, None),
        ("b_two", [(1, 1, 1), (4, 5, 1)], None, None),
        ("c_repeat", [(1, 1, 1), (1, 1, 1), (2, 1, 1)], None, None),
        ("d_diag", [(1, 1, 1), (2, 2, 2), (3, 3, 2), (4, 3, 2), (5, 3, 3), (6, 4, 3)], EX, None),
        ("e_2d", [(0, 0), (3, 4), (6, 4)], EX, None),
        ("f_bc", [(2, 1, 1), (4, 2, 1), (5, 4, 2), (5, 6, 4)], EX, bc_f),
        ("g_real", [(0.5, 1.25, 0.1), (1.7, 2.05, 0.35), (2.9, 1.15, 1.4), (4.45, 3.3, 1.85), (4.6, 3.35, 1.9)], EX, None),
        ("h_walk70", [tuple(int(v) for v in p) for p in walk], EX, None),
        ("i_long", [(3 * k, (k % 2) * 2, k // 3) for k in range(13)], None, None),
    ]
    out = dict(names=np.array([c[0] for c in cases]))
    paths, segs, times, keep, pts, ev_t, ev_p, checks, cons_rows, jerk_rows, bcs = [], [], [], [], [], [], [], [], [], [], []
    total, n_pts, opt_T, opt_total, opt_n, regen_total, regen_n = [], [], [], [], [], [], []
    for name, path, cons, bc in cases:
        tr = make(path, cons, bc)
        p = rows(tr.generate())
        dt = tr.constraints.min_time_step
        if name == "a_axis3":  # the repeated sum and k * dt give different counts here
            k = 0
            while k * dt <= tr.total_time:
                k += 1
            assert len(p) == 402 and k + (0 if (k - 1) * dt >= tr.total_time else 1) == 401
            assert tr.segment_times == [2.0, 2.0]
        paths.append(tr.path)
        segs.append(np.array(tr.segment_times, np.float64))
        total.append(float(tr.total_time))
        n_pts.append(len(p))
        times.append(p[:, 0].copy())
        idx = np.arange(len(p)) if len(p) <= 1500 else np.unique(np.concatenate(
            [np.arange(130), np.arange(0, len(p), 16), np.arange(len(p) - 130, len(p))]))
        keep.append(idx.astype(np.int32))
        pts.append(p[idx])
        cs = tr.check_constraints()
        checks.append([cs["velocity_satisfied"], cs["acceleration_satisfied"], cs["jerk_satisfied"]])
        cons_rows.append(list(tr.constraints.max_velocity) + list(tr.constraints.max_acceleration) + [dt])
        jerk_rows.append([NAN] * 3 if tr.constraints.max_jerk is None else list(tr.constraints.max_jerk))
        bcs.append(np.zeros((4, 3)) if bc is None else np.array(bc, np.float64))
        # evaluate(t): below 0, above total_time, on segment ends (the reference's start + duration) and
        # one ulp past them, mid-segment, total_time
        ends = [s.start_time + s.duration for s in tr.segments][:12]
        ts = [-0.5, 0.0] + ends + [float(np.nextafter(e, np.inf)) for e in ends] + [e - 0.37 for e in ends] + \
             [tr.total_time, tr.total_time + 2.0]
        ev_t.append(np.array(ts, np.float64))
        ev_p.append(rows([tr.evaluate(t) for t in ts]))
        if name == "d_diag":
            out["rs_case"] = np.int32(len(paths) - 1)
            out["rs_dt"] = np.float64(0.03)
            out["rs_pts"] = rows(tr.resample(0.03))
        # optimize_time_allocation(5) and the generate() after it (examples/3d_example.py:113-132)
        tr2 = make(path, cons, bc)
        tr2.optimize_time_allocation(max_iterations=5)
        opt_T.append(np.array(tr2.segment_times, np.float64))
        opt_total.append(float(tr2.total_time))
        opt_n.append(len(tr2.trajectory_points))
        q = rows(tr2.generate())
        regen_total.append(float(tr2.total_time))
        regen_n.append(len(q))
        assert np.array_equal(q, p, equal_nan=True) and tr2.segment_times == tr.segment_times
    checks = np.array(checks, bool)
    by = {c[0]: k for k, c in enumerate(cases)}
    assert not checks[by["b_two"], 1] and opt_total[by["b_two"]] > total[by["b_two"]]
    assert checks[by["d_diag"]].tolist() == [True, True, False]
    assert segs[by["c_repeat"]][0] == 0.5 and n_pts[by["i_long"]] >= 3000
    out["path"], out["path_off"] = ragged(paths, np.float64)
    out["path"] = out["path"].reshape(-1, 3)
    out["path_off"] = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    out["seg_times"], out["seg_off"] = ragged(segs, np.float64)
    out["times"], out["t_off"] = ragged(times, np.float64)
    out["pts_idx"], out["pts_off"] = ragged(keep, np.int32)
    out["pts"] = np.concatenate(pts)
    out["eval_t"], out["eval_off"] = ragged(ev_t, np.float64)
    out["eval_pts"] = np.concatenate(ev_p)
    out["opt_seg_times"], _ = ragged(opt_T, np.float64)
    out.update(cons=np.array(cons_rows, np.float64), max_jerk=np.array(jerk_rows, np.float64), bc=np.array(bcs, np.float64),
               total_time=np.array(total), n_pts=np.array(n_pts, np.int32), checks=checks,
               opt_total=np.array(opt_total), opt_n=np.array(opt_n, np.int32), regen_total=np.array(regen_total),
               regen_n=np.array(regen_n, np.int32))
    fn = os.path.join(HERE, "polytraj.npz")
    np.savez_compressed(fn, **out)
    print("polytraj cases", len(cases), "points", n_pts, "rows stored", len(out["pts"]), "bytes", os.path.getsize(fn))


if __name__ == "__main__":
    main()
