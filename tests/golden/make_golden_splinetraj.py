"""Generate tests/golden/splinetraj.npz by running the REFERENCE's SplineTrajectory3D
(trajectory/spline_trajectory.py:8-392, scipy's UnivariateSpline underneath) with pyvista and osqp
stubbed, as make_golden.py does.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_splinetraj.py

Per case: the path, the constraints, the degree, total_time before and after _enforce_constraints, its
two ratios and its scale, every time stamp, the rows (time, position, velocity, acceleration, yaw, yaw
rate; NaN = None) -- all of them for the short cases, the first and last 130 plus every 16th for the long
ones (pts_idx) -- u_waypoints, FITPACK's knots and coefficients per axis (_eval_args),
check_constraints(), the two ratios after scaling, evaluate(t) below 0, above total_time, at
total_time / 3, 0 and total_time; resample(0.03) and reparameterize_constant_speed() of the diagonal case.

A case is refused (AssertionError) when a discrete outcome would hang on a last bit: a sampling loop
whose last time at or below its total_time, or first time above it, is within 1e-9 relative of it; a
planar speed within 1e-3 relative of the 1e-6 yaw threshold; or FITPACK knots that are not bit-equal to
the fixed rule (k + 1 copies of u[0]; u[(k+1)/2 : n-(k+1)/2] for odd k, the midpoints
(u[j] + u[j+1]) / 2, j = k/2 .. n-k/2-2, for even k; k + 1 copies of u[-1])."""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, ragged  # noqa: E402

NAN = float("nan")
EX = ([2.0, 2.0, 1.5], [1.5, 1.5, 1.0], 0.05)  # examples/3d_example.py:104-109
DIAG = [(1, 1, 1), (2, 2, 2), (3, 3, 2), (4, 3, 2), (5, 3, 3), (6, 4, 3)]  # polytraj.npz's d_diag


def rows(pts):
    return np.array([[q.time, *q.position, *q.velocity, *q.acceleration, NAN if q.yaw is None else q.yaw,
                      NAN if q.yaw_rate is None else q.yaw_rate] for q in pts], np.float64).reshape(-1, 12)


def knots_rule(u, k):
    n = len(u)
    if k % 2:
        mid = list(u[(k + 1) // 2: n - (k + 1) // 2])
    else:
        mid = [(u[j] + u[j + 1]) / 2 for j in range(k // 2, n - k // 2 - 1)]
    return np.array([u[0]] * (k + 1) + mid + [u[-1]] * (k + 1))


def count_margin(total, dt, what):
    """the repeated sum's last time <= total and first time > total, both off total by > 1e-9 total"""
    t, last = 0.0, None
    while t <= total:
        last = t
        t += dt
    lo, hi = (total - last) / total, (t - total) / total
    assert lo > 1e-9 and hi > 1e-9, (what, lo, hi)
    return min(lo, hi)


def walk(rng, n):
    """n distinct lattice points, neighbours one step (of the 26) apart"""
    p, seen, out = np.array([40, 40, 20]), set(), []
    while len(out) < n:
        out.append(tuple(int(v) for v in p))
        seen.add(out[-1])
        while True:
            q = p + rng.integers(-1, 2, size=3)
            if tuple(int(v) for v in q) not in seen:
                p = q
                break
    return out


def main():
    import_reference()
    from python_motion_planning.trajectory import SplineTrajectory3D, TrajectoryConstraints

    rng = np.random.default_rng(11)
    loose = ([50.0, 50.0, 50.0], [400.0, 400.0, 400.0], 0.05)
    cases = [  # name, path, constraints (None = defaults), spline_degree (None = default)
        ("a_three", [(0, 0, 0), (2, 1, 0), (3, 3, 1)], None, None),
        ("b_four_k3", [(0, 0, 0), (1, 2, 0), (3, 3, 1), (4, 5, 3)], EX, 3),
        ("c_six_k5", [(0, 0, 0), (1, 2, 0), (3, 3, 1), (4, 5, 3), (6, 5, 4), (7, 7, 4)], EX, 5),
        ("d_five_k3", [(0, 0, 0), (1, 2, 0), (3, 3, 1), (4, 5, 3), (6, 5, 4)], EX, 3),
        ("e_seven_k5", [(0, 0, 0), (1, 2, 0), (3, 3, 1), (4, 5, 3), (6, 5, 4), (7, 7, 4), (9, 8, 6)], EX, 5),
        ("f_six_k4", [(2, 1, 1), (3, 3, 1), (5, 4, 2), (6, 6, 4), (8, 6, 5), (9, 8, 5)], EX, 4),
        ("g_five_k2", [(2, 1, 1), (3, 3, 1), (5, 4, 2), (6, 6, 4), (8, 6, 5)], EX, 2),
        ("h_diag_k3", DIAG, EX, 3),
        ("i_diag_k5", DIAG, EX, 5),
        ("j_2d", [(0, 0), (3, 4), (6, 4), (8, 7)], EX, 3),
        ("k_real", [(0.5, 1.25, 0.1), (1.7, 2.05, 0.35), (2.9, 1.15, 1.4), (4.45, 3.3, 1.85), (4.6, 3.35, 1.9)], EX, 3),
        ("l_anyangle", [(1, 1, 1), (2, 1, 1), (9, 6, 3), (11, 6, 3), (19, 14, 7), (20, 15, 7), (26, 15, 2)], EX, 3),
        ("m_walk64", walk(rng, 64), EX, 3),
        ("n_walk65", walk(rng, 65), EX, 5),
        ("o_loose", [(0, 0, 0), (1, 2, 0), (3, 3, 1), (4, 5, 3), (6, 5, 4)], loose, 3),
        ("p_short", [(0, 0, 0), (0.3, 0.2, 0.1), (0.5, 0.6, 0.2), (0.9, 0.7, 0.5)], ([2.0, 2.0, 1.5], [8.0, 8.0, 8.0], 0.05), 3),
        ("q_mid", [(0, 0, 0), (0.3, 0.2, 0.1), (0.5, 0.6, 0.2), (0.9, 0.7, 0.5)], ([2.0, 2.0, 1.5], [8.0, 8.0, 8.0], 0.01), 3),
    ]
    out = dict(names=np.array([c[0] for c in cases]))
    paths, times, keep, pts, ev_t, ev_p, uw, kn, co = [], [], [], [], [], [], [], [], []
    total, total0, n_pts, checks, cons_rows, degree, keff, ratios, ratios_after, scale, margins = ([] for _ in range(11))
    for name, path, cons, deg in cases:
        c = None if cons is None else TrajectoryConstraints(max_velocity=np.array(cons[0]), max_acceleration=np.array(cons[1]),
                                                            min_time_step=cons[2])
        kw = {} if deg is None else dict(spline_degree=deg)
        tr = SplineTrajectory3D(path=[tuple(p) for p in path], constraints=c, **kw)
        rec = {}
        orig = tr._enforce_constraints

        def spy(tr=tr, rec=rec, orig=orig):
            v, a = tr.get_velocities(), tr.get_accelerations()
            rec["T0"] = float(tr.total_time)
            rec["rv"] = float(np.max(np.abs(v) / tr.constraints.max_velocity))
            rec["ra"] = float(np.max(np.abs(a) / tr.constraints.max_acceleration))
            orig()
            rec["scale"] = float(tr.total_time) / rec["T0"] if tr.total_time != rec["T0"] else 1.0

        tr._enforce_constraints = spy
        p = rows(tr.generate())
        dt = tr.constraints.min_time_step
        k = tr.spline_degree
        # knots: bit-equal to the rule, for every axis
        for sp in tr.splines:
            t, cc, kk = sp._eval_args
            assert kk == k and np.array_equal(t, knots_rule(tr.u_waypoints, k)), (name, "knots")
        margins.append(count_margin(rec["T0"], dt, name))
        # yaw threshold
        sp_xy = np.sqrt(p[:, 4] ** 2 + p[:, 5] ** 2)
        assert np.all(np.abs(sp_xy - 1e-6) > 1e-9), (name, "yaw threshold")
        paths.append(tr.path)
        total.append(float(tr.total_time))
        total0.append(rec["T0"])
        ratios.append([rec["rv"], rec["ra"]])
        scale.append(rec["scale"])
        ratios_after.append([float(np.max(np.abs(p[:, 4:7]) / tr.constraints.max_velocity)),
                             float(np.max(np.abs(p[:, 7:10]) / tr.constraints.max_acceleration))])
        n_pts.append(len(p))
        times.append(p[:, 0].copy())
        idx = np.arange(len(p)) if len(p) <= 600 else np.unique(np.concatenate(
            [np.arange(130), np.arange(0, len(p), 16), np.arange(len(p) - 130, len(p))]))
        keep.append(idx.astype(np.int32))
        pts.append(p[idx])
        cs = tr.check_constraints()
        checks.append([cs["velocity_satisfied"], cs["acceleration_satisfied"], cs["jerk_satisfied"]])
        cons_rows.append(list(tr.constraints.max_velocity) + list(tr.constraints.max_acceleration) + [dt])
        degree.append(5 if deg is None else deg)
        keff.append(k)
        uw.append(np.array(tr.u_waypoints))
        kn.append(np.array(tr.splines[0]._eval_args[0]))
        co.append(np.array([sp._eval_args[1][: len(tr.path)] for sp in tr.splines]))
        ts = [-0.5, tr.total_time + 2.0, tr.total_time / 3, 0.0, tr.total_time]
        ev_t.append(np.array(ts, np.float64))
        ev_p.append(rows([tr.evaluate(t) for t in ts]))
        if name == "h_diag_k3":
            out["rs_case"] = np.int32(len(paths) - 1)
            out["rs_dt"] = np.float64(0.03)
            margins.append(count_margin(tr.total_time, 0.03, name + " resample"))
            out["rs_pts"] = rows(tr.resample(0.03))
            tr.reparameterize_constant_speed()
            margins.append(count_margin(tr.total_time, dt, name + " constant speed"))
            out["cs_pts"] = rows(tr.trajectory_points)
            out["cs_total"] = np.float64(tr.total_time)
    by = {c[0]: i for i, c in enumerate(cases)}
    ratios, n_pts, scale = np.array(ratios), np.array(n_pts, np.int32), np.array(scale)
    assert keff[by["a_three"]] == 2
    # the loose case: the reference does not scale, and not by a hair
    assert scale[by["o_loose"]] == 1.0 and np.all(ratios[by["o_loose"]] < 0.9)
    # one case scaled by the velocity ratio, one by the acceleration ratio
    sc = scale != 1.0
    assert np.any(sc & (ratios[:, 0] > np.sqrt(ratios[:, 1]))) and np.any(sc & (ratios[:, 0] < np.sqrt(ratios[:, 1])))
    assert np.any(n_pts < 64) and np.any((n_pts >= 64) & (n_pts <= 128)) and np.any(n_pts > 1000)
    assert len(paths[by["m_walk64"]]) == 64 and len(paths[by["n_walk65"]]) == 65
    out["path"], _ = ragged(paths, np.float64)
    out["path_off"] = np.concatenate([[0], np.cumsum([len(p) for p in paths])]).astype(np.int64)
    out["times"], out["t_off"] = ragged(times, np.float64)
    out["pts_idx"], out["pts_off"] = ragged(keep, np.int32)
    out["pts"] = np.concatenate(pts)
    out["u_waypoints"], _ = ragged(uw, np.float64)
    out["knots"], out["knot_off"] = ragged(kn, np.float64)
    out["coef"] = np.concatenate(co, axis=1)  # [3, sum n], case i's columns path_off[i] : path_off[i + 1]
    out["eval_t"] = np.array(ev_t, np.float64)
    out["eval_pts"] = np.array(ev_p, np.float64)
    out.update(cons=np.array(cons_rows, np.float64), degree=np.array(degree, np.int32), k=np.array(keff, np.int32),
               total_time=np.array(total), total_time_unscaled=np.array(total0), ratios=ratios,
               ratios_after=np.array(ratios_after), scale=scale, n_pts=n_pts, checks=np.array(checks, bool))
    fn = os.path.join(HERE, "splinetraj.npz")
    np.savez_compressed(fn, **out)
    print("splinetraj cases", len(cases), "points", n_pts.tolist(), "rows stored", len(out["pts"]), "bytes", os.path.getsize(fn))
    print("scale", scale.tolist())
    print("ratios", ratios.tolist())
    print("ratios after", np.array(ratios_after).tolist())
    print("smallest count margin", min(margins))


if __name__ == "__main__":
    main()
