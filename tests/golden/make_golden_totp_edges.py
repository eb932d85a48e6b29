"""Generate tests/golden/totp_edges.npz by running the REFERENCE's TimeOptimalTrajectory3D
(trajectory/time_optimal_trajectory.py:8-353) on the CPU, as make_golden.py's sec_totp does, on paths
chosen for the code of csrc/totp3d.hip that the grid paths of totp.npz never run.

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_totp_edges.py

Per named case: the path, the constraints (vmax, amax, min_time_step, path_resolution), total_time, the
four profiles, the point rows (all of them up to 1500, else every 10th and the last; NaN = None), n_pts,
and for some cases a list of times with the reference's evaluate(t) rows.  The layout is totp.npz's, so
golden_io.totp_compare's rule applies unchanged (tests/totp_checks.py).  The file is written with fixed
zip time stamps: the same reference gives the same bytes.

Every case asserts here what it is for (and tests/test_totp_edges_fixture.py asserts it again from the
file); the row exchanges of the spline solve are counted by totp_checks.exchanges, a numpy restatement of
the pivot comparisons of spline_slopes.

| case | what it is for |
|---|---|
| piv_mid | n = 8, uneven spacing: one exchange, at the interior step k = 3 |
| piv_last | n = 4: exchanges at k = 1 and at the last row, k = n - 2 = 2 |
| piv_run | n = 6: exchanges at k = 1, 2, 3, 4 (a run, the last row included) |
| piv3_a / piv3_b | n = 3 (the dense solve) with dx[1] > 1: rows 0 and 1 exchange / dx[1] < 1: none |
| noswap_uneven | n = 6, uneven spacing without an exchange (the control) |
| walk60 | 60 random non-integer waypoints (seed 60); its yaw also wraps inside rounds |
| big | coordinates near 1e4, limits of 20 / 10, path_resolution 2.0, min_time_step 0.5 |
| tiny | a path of 4 mm: 100 samples, 3 points |
| slow_axis | vmax_z = 0.05, amax_z = 0.02 decide the profile |
| fine | min_time_step = path_resolution = 0.01 |
| stuck | starts toward -x: the forward pass never leaves s_dot = 0, every yaw None, total_time = sum ds / 0.1 |
| ns128 / ns129 / ns130 | straight paths with those sample counts: the 64-wide profile rounds end on a full round less one, on a full round, and one past it |
| np64k | 128 points: the appended total_time is the last lane of a full round |
| np64k1_appended | 65 points: the appended total_time is alone in its round |
| np64k_exact | 128 points and none appended: a stuck straight path, whose total_time is a sum of ds / 0.1 that every implementation rounds alike, with min_time_step = total_time / 127 whose repeated sum lands on total_time exactly |
| yaw_wrap | leaves toward +x, turns round and runs toward -x while y wiggles: three pairs of consecutive yaws more than pi apart; the first is on row 256, the first row of a round, so its yaw rate uses the previous round's last point |
| yaw_gap | a vertical leg of 24 close waypoints: the spline's planar slope decays below 1e-6 / s_dot in its middle, so a run of None yaws lies strictly inside the trajectory |
| wp_limit | one path of totp_checks.MAX_WAYPOINTS waypoints, steps of about 0.1: the largest LDS block the entry accepts |

A yaw wrap on a multiple-of-64 row was obtained (yaw_wrap, first leg 2.5 long, row 256); walk60's wraps fall
inside rounds."""
from __future__ import annotations

import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import totp_checks as C  # noqa: E402
from make_golden import import_reference, ragged  # noqa: E402

NAN = float("nan")
EX = ([2.0, 2.0, 1.5], [1.5, 1.5, 1.0], 0.05, 0.05)  # examples/3d_example.py:104-109, :124-128
P0 = np.array([0.3, 0.1, 0.2])
DIR = np.array([0.8, 0.55, 0.2]) / np.linalg.norm([0.8, 0.55, 0.2])
EVAL_CASES = ("piv_run", "walk60", "ns129", "yaw_wrap", "piv3_a", "np64k_exact")


def rows(pts):
    return np.array([[q.time, *q.position, *q.velocity, *q.acceleration, NAN if q.yaw is None else q.yaw,
                      NAN if q.yaw_rate is None else q.yaw_rate] for q in pts], np.float64).reshape(-1, 12)


def run(path, cons, with_eval, seed):
    """make_golden.run_totp, plus evaluate(t) at the edges of its range and of time_profile's intervals"""
    from python_motion_planning.trajectory import TimeOptimalTrajectory3D, TrajectoryConstraints

    vmax, amax, tstep, res = cons
    tr = TimeOptimalTrajectory3D(path=[tuple(p) for p in path], path_resolution=res, constraints=TrajectoryConstraints(
        max_velocity=np.array(vmax), max_acceleration=np.array(amax), min_time_step=tstep))
    out = dict(pts=rows(tr.generate()), total_time=float(tr.total_time), s_values=np.asarray(tr.s_values, np.float64),
               s_dot=np.asarray(tr.s_dot_profile, np.float64), s_ddot=np.asarray(tr.s_ddot_profile, np.float64),
               time=np.asarray(tr.time_profile, np.float64), eval_t=np.zeros(0), eval_pts=np.zeros((0, 12)))
    if with_eval:
        T, tp = out["total_time"], out["time"]
        knots = [float(tp[k]) for k in (1, len(tp) // 2, len(tp) - 2)]
        ts = [-1.0, 0.0, T, T + 1.0, float(np.nextafter(T, 0.0))]
        for k in knots:
            ts += [k, float(np.nextafter(k, -np.inf)), float(np.nextafter(k, np.inf))]
        ts += (np.random.default_rng(seed).random(63) * T).tolist()
        assert len(ts) == 77 and all(0.0 < k < T for k in knots)
        out["eval_t"] = np.array(ts, np.float64)
        out["eval_pts"] = rows([tr.evaluate(t) for t in ts])
        assert np.isnan(out["eval_pts"][:, 10:]).all()
        assert out["eval_pts"][:5, 0].tolist() == [0.0, 0.0, T, T, ts[4]]
    return out


def straight(length, mid=None):
    pts = [P0] + ([P0 + mid * length * DIR] if mid else []) + [P0 + length * DIR]
    return np.array(pts, np.float64)


def limit_path(n):
    """n waypoints along a slow helix with uneven steps of about 0.1"""
    rng = np.random.default_rng(602)
    s = np.cumsum(rng.uniform(0.06, 0.14, n))
    return np.column_stack([4.0 * np.cos(s / 4.0) + 0.03 * s, 4.0 * np.sin(s / 4.0), 0.05 * s + 0.2 * np.sin(s / 3.0)])


def exact_path():
    """A straight path toward -x (stuck: total_time is the running sum of ds / 0.1 over np.linspace) whose
    total_time / 127, added up 127 times, gives total_time to the bit; the first of a fixed list of lengths.
    Returns (path, min_time_step)."""
    for j in range(200):
        length = 0.7 + 0.05 * j
        path = np.array([[0.5, 0.25, 0.125], [0.5 - length, 0.25 + 0.1 * length, 0.125]])
        ns, _ = C.n_samples_of(path, EX[3])
        sv = np.linspace(0, C.arc_lengths(path)[-1], ns)
        T = 0.0
        for k in range(1, ns):
            T = T + (sv[k] - sv[k - 1]) / 0.1
        ts, appended = C.step_times(T, T / 127)
        if not appended and len(ts) == 128:
            return path, T / 127
    raise AssertionError("no length lands on total_time")


def case_table():
    walk = np.cumsum(np.random.default_rng(60).uniform(-0.35, 0.35, size=(60, 3)) + [0.25, 0.1, 0.02], axis=0)
    a = 2.5  # yaw_wrap's first leg: the length that puts its first wrap on row 256
    up = [[3.0, 0.6, 0.2 + 0.1 * k] for k in range(1, 25)]
    exact, exact_dt = exact_path()
    return [
        ("piv_mid", [[0, 0, 0], [1, .2, 0], [2, .1, .3], [2.2, .2, .3], [2.3, .3, .4], [5.5, 1, 1], [6.5, 1.5, 1.2], [7.5, 2.5, 1.0]], EX),
        ("piv_last", [[0, 0, 0], [.1, 0, 0], [.2, .1, 0], [6, 3, 1]], EX),
        ("piv_run", [[0, 0, 0], [.1, 0, 0], [.3, .1, 0], [1.3, .1, .2], [5, 1, 1], [20, 3, 2]], EX),
        ("piv3_a", [[0, 0, 0], [.4, .2, 0], [3, 1, .5]], EX),
        ("piv3_b", [[0, 0, 0], [2.4, .9, .3], [3, 1, .5]], EX),
        ("noswap_uneven", [[0, 0, 0], [1.3, .2, 0], [2, .9, .1], [3.7, 1.1, .4], [4.6, 2.0, .5], [6.1, 2.2, .9]], EX),
        ("walk60", walk, EX),
        ("big", 1e4 + np.array([[0, 0, 0], [31.5, 4.2, 1], [55.1, 22.7, 3.5], [90.2, 31, 9.1], [120.7, 28.3, 12.2], [160.1, 40.9, 10.4]]),
         ([20.0, 20.0, 15.0], [10.0, 10.0, 8.0], 0.5, 2.0)),
        ("tiny", 1e-3 * np.array([[0, 0, 0], [1.3, .2, 0], [2, .9, .1], [3.7, 1.1, .4]]), EX),
        ("slow_axis", [[0, 0, 0], [1.3, .2, .1], [2, .9, .15], [3.7, 1.1, .3]], ([2.0, 2.0, 0.05], [1.5, 1.5, 0.02], 0.05, 0.05)),
        ("fine", [[0, 0, 0], [1.1, .2, .1], [1.9, .9, .15], [2.7, 1.1, .3]], ([2.0, 2.0, 1.5], [1.5, 1.5, 1.0], 0.01, 0.01)),
        ("stuck", [[0, 0, 0], [-1.5, .2, 0], [-3, -.2, .5]], EX),
        ("ns128", straight(6.42), EX),
        ("ns129", straight(6.47, mid=0.37), EX),
        ("ns130", straight(6.52), EX),
        ("np64k", straight(12.361), EX),
        ("np64k1_appended", straight(4.561), EX),
        ("np64k_exact", exact, (EX[0], EX[1], exact_dt, EX[3])),
        ("yaw_wrap", [[0, 0, 0], [a, .3, 0], [a + 1.2, 1.5, 0], [a + .4, 2.9, 0], [a - 1.5, 3.2, 0], [a - 3, 2.9, 0], [a - 4.5, 3.25, 0],
                      [a - 6, 2.95, 0]], EX),
        ("yaw_gap", [[0, 0, 0], [1.5, .4, .05], [3.0, .6, .2]] + up + [[3.6, 1.0, up[-1][2] + .3], [5, 1.6, up[-1][2] + .5]], EX),
        ("wp_limit", limit_path(C.MAX_WAYPOINTS), EX),
    ]


def count_margin(r, dt):
    """total_time - the last repeated-sum time, which must be clear of 0 and of dt for the point count to be
    a property of the arithmetic and not of its last bit"""
    ts, appended = C.step_times(r["total_time"], dt)
    gap = r["total_time"] - ts[-1]
    assert len(ts) + appended == len(r["pts"])
    assert appended == (r["pts"][-2, 0] + dt > r["total_time"])
    return gap, appended


def check(name, path, cons, r):
    """What the case is for"""
    dt, res = cons[2], cons[3]
    ex = C.exchanges(path)
    n, pts, T = len(path), r["pts"], r["total_time"]
    nan = np.isnan(pts[:, 10])
    want_ex = dict(piv_mid=[3], piv_last=[1, 2], piv_run=[1, 2, 3, 4], piv3_a=[0], piv3_b=[], noswap_uneven=[])
    if name in want_ex:
        assert ex == want_ex[name], (name, ex)
        assert (n == 3) == name.startswith("piv3") and (n >= 4) == (not name.startswith("piv3"))
    if name.startswith("piv3"):
        d1 = np.diff(C.arc_lengths(path))[1]
        assert (d1 > 1.0) == (name == "piv3_a")
    if name == "noswap_uneven":
        d = np.diff(C.arc_lengths(path))
        assert d.max() / d.min() > 1.5
    if name == "walk60":
        assert n == 60 and not np.any(path == np.round(path))
    if name == "big":
        assert np.min(np.abs(path)) >= 1e4 and res == 2.0
    if name == "tiny":
        assert len(r["s_values"]) == 100 and len(pts) == 3 and C.arc_lengths(path)[-1] < 5e-3
    if name == "slow_axis":
        assert C.slow_axis_dominates(pts, cons[0])
    if name == "fine":
        assert dt == res == 0.01
    if name == "stuck":
        sv = r["s_values"]
        tot = 0.0
        for k in range(1, len(sv)):
            tot = tot + (sv[k] - sv[k - 1]) / 0.1
        assert r["s_dot"].max() == 0.0 and nan.all() and T == tot and path[1][0] < path[0][0]
    if name in ("ns128", "ns129", "ns130"):
        ns, q = C.n_samples_of(path, res)
        assert ns == int(name[2:]) == len(r["s_values"]) and 1e-6 < q - int(q) < 1 - 1e-6
        assert n == (3 if name == "ns129" else 2)
    if name in ("np64k", "np64k1_appended", "np64k_exact", "ns128", "ns129", "ns130", "tiny"):  # a count at stake
        gap, appended = count_margin(r, dt)
        if name == "np64k_exact":
            assert not appended and gap == 0.0 and pts[-1, 0] == T and len(pts) % 64 == 0 and r["s_dot"].max() == 0.0
        else:
            assert appended and pts[-1, 0] == T
            assert 1e-9 * T < gap < dt - 1e-9 * T, (name, gap)
        if name == "np64k":
            assert len(pts) % 64 == 0 and len(pts) >= 128
        if name == "np64k1_appended":
            assert len(pts) % 64 == 1 and len(pts) >= 65
    if name == "yaw_wrap":
        w = C.yaw_wraps(pts)
        assert np.all(path[:, 2] == 0.0) and path[1][0] > path[0][0] and path[-1][0] < path[-2][0]
        assert len(w) >= 1 and w[0] == 256, w
        for k in w:  # clear of the branch cut: a wrap there is no rounding accident
            assert np.pi - abs(pts[k, 10]) > 1e-3 and np.pi - abs(pts[k - 1, 10]) > 1e-3
    if name == "yaw_gap":
        edges = np.nonzero(np.diff(nan.astype(int)))[0] + 1
        inside = [(a, b) for a, b in zip(edges[:-1], edges[1:]) if nan[a] and a > 0 and b < len(pts) and not nan[a - 1] and not nan[b]]
        assert inside and inside[0][1] - inside[0][0] >= 3, edges
        assert nan.any() and (~nan).any()
    if name == "wp_limit":
        assert n == C.MAX_WAYPOINTS == 602 and C.lds_bytes(n) <= C.LDS_BYTES < C.lds_bytes(n + 1)
        assert 1000 <= len(r["s_values"]) <= 1400


def save_npz(fn, arrays):
    """np.savez_compressed with fixed member time stamps: the same arrays give the same bytes"""
    with zipfile.ZipFile(fn, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    import_reference()
    cases, res = [], []
    for k, (name, path, cons) in enumerate(case_table()):
        path = np.asarray(path, np.float64)
        r = run(path, cons, name in EVAL_CASES, 1000 + k)
        check(name, path, cons, r)
        cases.append((name, path, cons))
        res.append(r)
    keep = [np.arange(len(r["pts"])) if len(r["pts"]) <= 1500 else
            np.unique(np.append(np.arange(0, len(r["pts"]), 10), len(r["pts"]) - 1)) for r in res]
    out = dict(names=np.array([c[0] for c in cases]))
    out["path"], _ = ragged([c[1] for c in cases], np.float64)
    out["path"] = out["path"].reshape(-1, 3)
    out["path_off"] = np.concatenate([[0], np.cumsum([len(c[1]) for c in cases])]).astype(np.int64)
    out["cons"] = np.array([list(c[2][0]) + list(c[2][1]) + [c[2][2], c[2][3]] for c in cases], np.float64)
    out["total_time"] = np.array([r["total_time"] for r in res])
    out["prof_off"] = np.concatenate([[0], np.cumsum([len(r["s_values"]) for r in res])]).astype(np.int64)
    for k in C.PROFILES:
        out[k] = np.concatenate([r[k] for r in res])
    out["pts_off"] = np.concatenate([[0], np.cumsum([len(k) for k in keep])]).astype(np.int64)
    out["pts"] = np.concatenate([r["pts"][k] for r, k in zip(res, keep)])
    out["pts_idx"] = np.concatenate(keep).astype(np.int32)
    out["n_pts"] = np.array([len(r["pts"]) for r in res], np.int32)
    out["eval_t"], out["eval_off"] = ragged([r["eval_t"] for r in res], np.float64)
    out["eval_pts"] = np.concatenate([r["eval_pts"] for r in res])
    fn = os.path.join(HERE, "totp_edges.npz")
    save_npz(fn, out)
    print("totp_edges cases", len(cases), "samples", out["prof_off"][-1], "points", out["n_pts"].tolist(), "rows stored",
          len(out["pts"]), "bytes", os.path.getsize(fn))


if __name__ == "__main__":
    main()
